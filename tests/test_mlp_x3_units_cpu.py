"""CPU side of the unit-level harness of dhaug_mlp_forward_x3 (tests/mlp_x3_unit_util.py): every program the GPU test runs is
built and referenced here and held to the conditions that make its bit-for-bit comparison legitimate -- for every GEMM unit, row
and feature, none excluded: sum|terms| < 2^22 q over the three kept product terms, the bias and the residual; every stored
activation equal to its hi + lo and below 65 504; every non-zero piece a normal fp16 number -- and to non-degenerate outputs.
Then what the families claim to cover (all 36 (chunks, map, add-mode) instantiations of either layer body), the numpy packers
against the header's formula, and the planner's refusals, which need no GPU: dhaug_mlp_forward_x3 validates and plans a program
before it launches anything, so the pointers are host memory that nothing dereferences."""
import ctypes
import os
import sys

import numpy as np
import pytest

import mlp_unit_util as U
import mlp_x3_unit_util as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_EXACT = [n for f in X.TIER1 + ("cap", "ship") for n in X.names(f)]


@pytest.mark.parametrize("name", ALL_EXACT)
def test_program_is_exact_and_not_degenerate(name):
    p = X.get(name)
    r = X.walk(p)                                                             # asserts every condition for every unit, afresh
    assert p.tier == 1 and 0 < r["bits"] < X.EXACT_BITS
    assert all(not b.any() for b in r["bound"].values())
    X.nondegenerate(p)
    for T in p.tensors.values():                                              # every output sits in a wider tensor
        if T["data"] is None and not name.startswith("ship_"):              # (the shipped builders allocate their own outputs)
            assert T["ld"] > T["width"]
    if p.fam == "tp":                                                         # the lo planes and both cross terms hold content
        g = [u for u in p.units if u["kind"] == X.GEMM and not u.get("select")]
        assert any(X.split(u["W"])[1].any() for u in g), "no weight has a lo piece"
        assert any(X.split(T["data"])[1].any() for T in p.tensors.values() if T["data"] is not None), "no input has a lo piece"
    else:
        for T in p.tensors.values():
            assert T["data"] is None or X.is_f16(X.kcs_features(T["data"]) if T["kcs"] else T["data"])
        assert all(X.is_f16(u["W"]) for u in p.units if u["kind"] == X.GEMM and u["W"] is not None)


@pytest.mark.parametrize("name", X.names("real"))
def test_realistic_programs_have_finite_positive_bounds(name):
    p = X.get(name)
    r = p.ref()
    assert p.tier == 2 and p.mmax == 129
    for t, b in r["bound"].items():
        assert np.isfinite(b).all() and (b > 0).all() and np.isfinite(r["out"][t]).all()
        # (3 K + 2) 2^-24 S dominates: 4e-5 at K = 50, 5e-4 at K = 256 for outputs of order 1
        assert np.median(b) < 1e-3 * np.abs(r["out"][t]).max()


def test_the_families_cover_what_they_claim():
    full = {(c, m, a) for c in (1, 2, 4) for m in (X.MAP_1x4, X.MAP_1x2, X.MAP_1x1) for a in X.ADD_MODES}
    for t16 in (False, True):
        tier1 = set()
        for n in ALL_EXACT:
            p = X.get(n)
            if p.t16 == t16 and not n.startswith("ship_"):
                tier1 |= {(g["chunks"], g["map"], g["add"]) for g in p.ref()["plan"]}
        assert tier1 == full, sorted(full - tier1)                            # all 36 of the dispatch switch, without the builders
        for fam in ("int", "tp"):
            singles = [X.get(n) for n in X.names("single") if X.get(n).t16 == t16 and X.get(n).fam == fam]
            g = [p.units[1] for p in singles]
            assert {(u["K"], u["N"]) for u in g} >= {(K, N) for K in X.K1 for N in X.N1}
            for K in X.K1:
                assert {u["act"] for u in g if u["K"] == K} == {0, 1, 2}
            for N in X.N1:
                assert {u["act"] for u in g if u["N"] == N} == {0, 1, 2}
                if N <= 64:
                    assert {bool(u["flags"] & X.F_OUT_F32) for u in g if u["N"] == N} == {True, False}
            assert {p.tensors["x"]["ld"] > p.tensors["x"]["width"] for p in singles} == {True, False}
        real = {(g["chunks"], g["map"]) for n in X.names("real") if X.get(n).t16 == t16 for g in X.get(n).ref()["plan"][:1]}
        assert real == {(c, m) for c in (1, 2, 4) for m in (1, 2, 3)}
        # a parking unit, a parked sum added in every map, a stash added in every map
        plans = [g for n in ALL_EXACT if X.get(n).t16 == t16 for g in X.get(n).ref()["plan"]]
        assert {g["map"] for g in plans if g["pf"] & X.PF_TO_PARK} == {1, 2, 3}
    assert {n.split("_")[0] for n in X.names("cap")} == {"single", "res", "park", "kcs", "stale"}
    assert all(X.get(n).mmax == X.M_CAP and X.get(n).cap == 2 for n in X.names("cap"))
    ships = X.names("ship")
    assert {n[:-4] for n in ships} >= {"ship_%s_D%d_int" % (k, D) for k in ("gen", "d2", "d3") for D in (64, 128, 256)}


def test_reference_orders_the_epilogue_as_the_kernel_does():
    """a parking unit stores act(v) and leaves the image; the parked sum and the residual are added before the activation"""
    p = X.Program("t", 1)
    p.inp("a", 30)
    p.load("a", 1)
    p.gemm(1, 0, 48, 30, X.NONE, W=np.eye(48, 30), b=np.zeros(48))            # the image holds a
    p.gemm(0, 2, 35, 48, X.RELU, W=-np.eye(35, 48), b=np.zeros(35))           # parked: relu(-a)
    p.gemm(0, 2, 35, 48, X.RELU, W=np.eye(35, 48), b=np.full(35, -1.0), res=2)   # the image still holds a: relu(a - 1 + relu(-a))
    p.observe(2, 35)
    r = p.ref()
    a = p.tensors["a"]["data"]
    want = np.zeros((p.mmax, 35))
    want[:, :30] = np.maximum(a - 1.0 + np.maximum(-a, 0.0), 0.0)
    assert np.array_equal(r["out"]["y"], want)
    assert [g["pf"] for g in r["plan"]] == [0, X.PF_TO_PARK, X.PF_ADD_R1, 0]


def test_reference_refuses_what_the_planner_refuses():
    def prog(build):
        p = X.Program("t", 2)
        p.inp("x", 64)
        p.load("x", 1)
        build(p)
        with pytest.raises(X.Refused) as e:
            p.ref()
        return e.value.code

    def clobbered(p):                                                         # the second adder would find the first adder's result
        p.gemm(1, 0, 256, 64)
        p.gemm(0, 1, 256, 256)
        p.gemm(1, 2, 256, 256, res=0)
        p.gemm(2, 1, 256, 256)
        p.gemm(1, 2, 256, 256, res=0)
        p.observe(2, 256)

    def groups(p):                                                            # kept on eight waves (N = 64), added on four (N = 20)
        p.gemm(1, 0, 64, 64)
        p.gemm(0, 1, 64, 64)
        p.gemm(1, 2, 20, 64, res=0)
        p.observe(2, 20)

    def not_image(p):
        p.gemm(2, 0, 64, 64)
        p.observe(0, 64)

    assert prog(clobbered) == prog(groups) == prog(not_image) == X.EUNSUPPORTED


def _loop_pack(W, K, k0, t16):
    N = W.shape[0]
    ksteps = 4 * ((K + 63) // 64)
    out = np.zeros(2 * 8 * ksteps * 512)
    for i in range(8 * ksteps * 512):
        j, lane, blk = i & 7, (i >> 3) & 63, i >> 9
        if t16:
            kt = ksteps // 2
            ks, ft, s = blk % kt, (blk // kt) & 1, blk // (2 * kt)
            n, k = 32 * s + 16 * ft + (lane & 15), 32 * ks + 8 * (lane >> 4) + j
        else:
            ks, s = blk % ksteps, blk // ksteps
            n, k = 32 * s + (lane & 31), 16 * ks + 8 * (lane >> 5) + j
        w = W[n, k0 + k] if (n < N and k < K) else 0.0
        hi = float(np.float16(np.float32(w)))
        o = ((blk * 2) * 64 + lane) * 8 + j
        out[o], out[o + 512] = hi, float(np.float16(np.float32(w - hi)))
    return out


@pytest.mark.parametrize("t16", [False, True])
def test_numpy_packers_follow_the_header_formula(t16):
    rng = np.random.default_rng(5)
    W = rng.standard_normal((37, 150)).astype(np.float32).astype(np.float64)
    W[3, 7], W[4, 60] = 1.0 + 2.0 ** -11, -0.0
    for K, k0 in ((100, 0), (64, 50), (9, 141)):
        blob = X.pack_f16x2(W, K, k0, t16)
        assert blob.shape == (2 * 8 * 4 * ((K + 63) // 64) * 512,)
        assert np.array_equal(blob.view(np.float16).astype(np.float64), _loop_pack(W, K, k0, t16))
        assert np.count_nonzero(blob.view(np.float16)[np.arange(blob.size) // 512 % 2 == 1]) > 0          # lo blocks hold content
    hi, lo = X.split(np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0, 3.0 + 2.0 ** -11]))
    assert hi.tolist() == [1.0, 1.0 + 2.0 ** -9, 0.0, 3.0] and lo.tolist() == [2.0 ** -11, -2.0 ** -11, 0.0, 2.0 ** -11]   # ties to even


def test_conditions_refuse_what_the_pair_cannot_hold():
    X.pieces_ok("t", np.array([3.0 + 2.0 ** -11, 0.0, -2.0 ** -14, 1024.0 + 2.0 ** -11]))
    with pytest.raises(AssertionError, match="22 bits"):
        X.pieces_ok("t", np.array([1.0 + 2.0 ** -11 + 2.0 ** -23]))       # hi = 1 + 2^-10, the rest needs 12 bits
    with pytest.raises(AssertionError, match="normal fp16"):
        X.pieces_ok("t", np.array([1.0 + 2.0 ** -15]))                        # lo = 2^-15: a subnormal piece
    with pytest.raises(AssertionError, match="fp16 range"):
        X.pieces_ok("t", np.array([65504.0]))
    with pytest.raises(AssertionError, match="no fp16 value"):
        U._exactness("t", np.array([[1.0 + 2.0 ** -11]]), np.array([[1.0]]), [], fmt=X.is_f16, fmt_name="fp16")
    with pytest.raises(AssertionError, match="below 2\\^22"):                 # Whi Xlo of 2^-23 granularity beside integers
        U._exactness("t", np.array([[4.0, 2.0 ** -12]]), np.array([[1.0, 1.0 + 2.0 ** -10]]), [], fmt=X.is_f16)
    f = X.kcs_features(X.axis_poses(np.random.default_rng(1), 50))
    assert f.shape == (50, 30) and np.isin(f[:, :15], (-1.0, 0.0, 1.0)).all() and (f[:, 15:] >= 1).all() and X.is_f16(f)
    assert len({tuple(r) for r in f}) == 50


# ---- the planner's refusals -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd  # noqa: F401
    from dhaug_amd import _lib
    return _lib


def test_planner_refuses_with_the_code_the_source_gives(lib):
    L = lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ptr = ctypes.c_void_p(base)
    EINVAL, EALIGN, EUNSUPPORTED = X.EINVAL, X.EALIGN, X.EUNSUPPORTED

    def unit(kind, **kw):
        u = lib.MlpUnit()
        u.kind, u.src, u.dst, u.res, u.src2 = kind, -1, -1, -1, -1
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def run(*units, n=None):
        arr = (lib.MlpUnit * max(len(units), 1))(*units)
        n = len(units) if n is None else n
        rc = L.dhaug_mlp_forward_x3(arr, n, 128, None)
        if 1 <= n <= 32:
            assert L.dhaug_mlp_forward_x3(arr, n, 0, None) == 0              # an empty batch looks at no unit
        return rc

    load = lambda **kw: unit(X.LOAD_F32, **dict(dict(dst=1, cols=64, ld=64, g=ptr), **kw))
    gemm = lambda **kw: unit(X.GEMM, **dict(dict(src=1, dst=0, ksteps=4, n=256, w=ptr, bias=ptr, g=ptr), **kw))
    out = lambda **kw: gemm(**dict(dict(flags=X.F_OUT_F32, n=35, ld=40), **kw))
    # a GEMM whose source is not what the image holds
    assert run(load(), gemm(src=2)) == EUNSUPPORTED
    assert run(load(), gemm(), gemm(src=1, dst=2)) == EUNSUPPORTED            # (the first layer overwrote buffer 1's value)
    # a residual that is in neither the stash nor region 1
    assert run(load(), gemm(res=2)) == EUNSUPPORTED
    assert run(load(), gemm(), gemm(src=0, dst=1, ksteps=16, res=2)) == EUNSUPPORTED
    # a stash / region-1 value added under a different map than it was written with
    assert run(load(), gemm(), gemm(src=0, dst=1, ksteps=16, n=100), gemm(dst=2, ksteps=7, n=100, res=0)) == EUNSUPPORTED
    assert run(load(), gemm(n=64), gemm(src=0, dst=1, n=64), gemm(dst=2, n=20, res=0)) == EUNSUPPORTED       # (eight waves / four)
    assert run(load(), gemm(), gemm(src=0, dst=2, ksteps=16, n=100), load(), gemm(),
               gemm(src=0, dst=2, ksteps=16, n=225, res=2)) == EUNSUPPORTED
    # a second value parked while one waits
    assert run(load(), gemm(), gemm(src=0, dst=2, ksteps=16, n=100), gemm(src=0, dst=1, ksteps=16, n=100),
               gemm(src=0, dst=2, ksteps=16, n=100, res=2), gemm(src=2, dst=0, ksteps=7, n=100, res=1)) == EUNSUPPORTED
    # an adding layer always keeps its result: it may not overwrite a stash value that is added once more
    assert run(load(), gemm(), gemm(src=0, dst=1, ksteps=16), gemm(dst=2, ksteps=16, res=0), gemm(src=2, dst=1, ksteps=16),
               gemm(dst=2, ksteps=16, res=0)) == EUNSUPPORTED
    for ks in (9, 10, 11, 12):                                                # K of 129..192: three chunks
        assert run(load(), gemm(ksteps=ks)) == EUNSUPPORTED
    assert run(load(), gemm(n=257)) == EUNSUPPORTED
    assert run(load(), out(n=65, ld=72)) == EUNSUPPORTED
    assert run(load(), out(n=35, ld=34)) == EUNSUPPORTED
    assert run(load(), gemm(n=64), gemm(src=0, dst=1, n=64), out(dst=2, n=64, ld=64, res=0)) == EUNSUPPORTED  # OUT_F32 + residual
    assert run(load(), gemm(ksteps2=4, src2=2, w2=ptr)) == EUNSUPPORTED
    assert run(load(), gemm(flags=X.F_T16), gemm(src=0, dst=1, ksteps=16)) == EINVAL                        # one layout per program
    assert run(load(), gemm(), gemm(src=0, dst=1, ksteps=16, flags=X.F_T16)) == EINVAL
    for flag in (1, 2, 8, 16, 64):                                            # an unknown flag (16: DOT_OUT, the bf16 kernel's)
        assert run(load(), gemm(flags=flag)) == EUNSUPPORTED
    assert run(load(), gemm(w=ctypes.c_void_p(base + 8))) == EALIGN
    assert run(load(), gemm(bias=ctypes.c_void_p(base + 4))) == EALIGN
    assert run(load(), gemm(g=ctypes.c_void_p(base + 8))) == EALIGN           # (the workspace)
    assert run(load(cols=63), gemm()) == EALIGN
    assert run(load(ld=65), gemm()) == EALIGN
    assert run(load(g=ctypes.c_void_p(base + 4)), gemm()) == EALIGN
    assert run(load(cols=0), gemm()) == EINVAL
    assert run(load(cols=258, ld=258), gemm()) == EINVAL
    assert run(load(cols=64, ld=62), gemm()) == EALIGN                        # (ld < cols is reported with the pitch checks)
    assert run(unit(X.LOAD_KCS, dst=1, ld=46, g=ptr), gemm()) == EINVAL
    assert run(load()) == EINVAL                                              # no GEMM unit
    assert run(load(), unit(X.LOAD_KCS, dst=0, ld=48, g=ptr)) == EINVAL
    assert run(n=0) == EINVAL and run(*([load()] + [gemm()] + [load()] * 31), n=33) == EINVAL
    assert L.dhaug_mlp_forward_x3(None, 2, 0, None) == EINVAL
    assert run(unit(7, dst=1), gemm()) == EUNSUPPORTED                        # no such unit kind (STORE_BF16 = 2 likewise)
    assert run(unit(2, src=1, cols=64, ld=64, g=ptr), gemm()) == EUNSUPPORTED
