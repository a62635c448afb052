"""Programs for the route "stack with its lead operand from global memory" of dhaug_mlp_forward (csrc/dhaug_mlp.hip, PLAN_LEADG):
a bf16 LOAD of 32 or 48 columns that feeds nothing but the lead layer of a stack runs as one unit with that stack, and the lead
reads its MFMA B fragments from the tensor itself.  Built on tests/mlp_unit_util.py (Program, the fp64 reference, the exactness
condition); none of them is registered there, so the existing parametrisations are what they were.

The route is refused for programs with a STORE (their LOADs may need the drain barrier), so every program here leaves through an
fp32 output or a DOT_OUT logit.  NOLEADG in the environment switches the route off in the planner; plans() asks the library which
route a program gets (dhaug_mlp_plan: host only, nothing is launched, no pointer is dereferenced)."""
import contextlib
import ctypes
import os

import numpy as np

import mlp_unit_util as U

NOLEADG = "DHAUG_MLP_NOLEADG"
PLAN_STACK, PLAN_LEADG = 1 << 13, 1 << 15
MS = (1, 31, 33, 127, 128, 129, 300)
GUARD = 16                                        # NaN elements in front of an input, behind it, and behind each row where ld > cols


@contextlib.contextmanager
def route(on):
    old = os.environ.pop(NOLEADG, None)
    try:
        if not on:
            os.environ[NOLEADG] = "1"
        yield
    finally:
        os.environ.pop(NOLEADG, None)
        if old is not None:
            os.environ[NOLEADG] = old


# ---- builders: (ld_extra, dtype of the lead's input, D, attempt) -> Program ------------------------------------------------
def _prog(name, attempt, mmax, cap):
    return U.Program(name, U._seed(name) + attempt, mmax=mmax, cap=cap)


def _run(p, n, respat, acts, src=0, D=256):
    """n full-width layers alternating between buffers 0 and 1, first source `src`; returns the buffer that holds the result"""
    for j in range(n):
        has_res = (respat == "odd" and j % 2 == 1) or (respat == "even" and j % 2 == 0)
        p.gemm(src, 1 - src, D, D, acts[j % len(acts)], res=(1 - src) if has_res else -1, ksteps=(D + 15) // 16, nnz=6)
        src = 1 - src
    return src


def l32_r2(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    """bf16 LOAD of 32 columns + lead + run of 2 (ReLU) + fp32 output"""
    p = _prog("leadg_l32_r2", attempt, mmax, cap)
    p.inp("x", 32, dtype, ld=32 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 32, U.RELU)
    src = _run(p, 2, "none", (U.RELU,), D=D)
    p.gemm(src, 1 - src, 35, D, U.NONE, out="y", ksteps=(D + 15) // 16)
    return p


def l48_r3(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    """48 columns + run of 3 with odd residuals + fp32 tail N = 1"""
    p = _prog("leadg_l48_r3", attempt, mmax, cap)
    p.inp("x", 48, dtype, ld=48 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 48, U.RELU)
    src = _run(p, 3, "odd", (U.RELU,), D=D)
    p.gemm(src, 1 - src, 1, D, U.NONE, out="y", ksteps=(D + 15) // 16)
    return p


def l32_r7_leaky(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    """32 columns + run of 7, LeakyReLU, odd residuals, bf16 tail into buffer 2 with a residual from there; one more layer reads
    buffer 2 out as fp32"""
    p = _prog("leadg_l32_r7_leaky", attempt, mmax, cap)
    p.inp("r2", 128, "bf16", lo=-6, hi=6)
    p.load("r2", 2)
    p.inp("x", 32, dtype, ld=32 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 32, U.LRELU)
    src = _run(p, 7, "odd", (U.LRELU,), D=D)
    p.gemm(src, 2, 128, D, U.RELU, res=2, ksteps=(D + 15) // 16)
    p.gemm(2, 0, 64, 128, U.NONE, out="y")
    return p


def d3_shaped(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0, name="leadg_d3"):
    """the 3D critic's program (fused._d3_program) with both inputs bf16: two fused places, the parked merge half between them"""
    p = _prog(name, attempt, mmax, cap)

    def blocks():
        for _ in range(3):
            p.gemm(0, 1, D, D, U.RELU, nnz=6, ksteps=(D + 15) // 16)
            p.gemm(1, 0, D, D, U.RELU, res=0, nnz=6, ksteps=(D + 15) // 16)

    p.inp("kcs", 32, "bf16", ld=32 + lde)
    p.load("kcs", 1)
    p.gemm(1, 0, D, 30, U.RELU)
    blocks()
    p.gemm(0, 2, 100, D, U.NONE, nnz=4, ksteps=(D + 15) // 16)              # merge layer, KCS half: parked in buffer 2
    p.inp("x", 48, dtype, ld=48 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 48, U.RELU)
    blocks()
    p.gemm(0, 2, 100, D, U.RELU, res=2, nnz=4, b=np.zeros(100), ksteps=(D + 15) // 16)
    p.gemm(2, 0, 100, 100, U.RELU)
    p.gemm(0, 1, 100, 100, U.RELU, res=2, dot="y")
    return p


def d3_cap(lde=0, dtype="bf16", D=256, attempt=0):
    """M = 643 on two workgroups: three tiles each, the ragged one last"""
    return d3_shaped(lde, dtype, D, attempt, mmax=U.M_CAP, cap=2, name="leadg_d3_cap")


def d2_shaped(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    """the 2D critic's program (fused._d2_program, composed form: three wide layers behind the lead, fp32 logit)"""
    p = _prog("leadg_d2", attempt, mmax, cap)
    ks = (D + 15) // 16
    p.inp("x", 32, dtype, ld=32 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 32, U.LRELU)
    p.gemm(0, 1, D, D, U.LRELU, nnz=6, ksteps=ks)
    p.gemm(1, 0, D, D, U.LRELU, res=0, nnz=6, ksteps=ks)
    p.gemm(0, 1, D, D, U.LRELU, nnz=6, ksteps=ks)
    p.gemm(1, 0, 1, D, U.NONE, out="y", ksteps=ks)
    return p


# the refused shapes: they keep the LOAD unit
def refused_even(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    """the first run layer adds its residual in place to the buffer the LOAD wrote: columns [0, 64) of it are the LOAD's image"""
    p = _prog("leadg_refused_even", attempt, mmax, cap)
    p.inp("r", 256, "bf16", lo=-3, hi=3)
    p.load("r", 1)
    p.inp("x", 32, dtype, ld=32 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 32, U.RELU)
    src = _run(p, 3, "even", (U.RELU,), D=D)
    p.gemm(src, 1 - src, 35, D, U.NONE, out="y", ksteps=(D + 15) // 16)
    return p


def refused_store(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    """a program with a STORE and a LOAD of the parked rows: its bf16 LOADs wait for the workgroup's stores"""
    p = _prog("leadg_refused_store", attempt, mmax, cap)
    p.inp("x", 48, dtype, ld=48 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 48, U.RELU)
    src = _run(p, 2, "odd", (U.RELU,), D=D)                                  # result in buffer 0
    p.store(src, 32, "park", ld=40)
    p.load("park", 1)                                                        # 32 parked columns feed a lead again
    p.gemm(1, 0, D, 32, U.RELU)
    src = _run(p, 2, "none", (U.RELU,), D=D)
    p.gemm(src, 1 - src, 35, D, U.NONE, out="y", ksteps=(D + 15) // 16)
    return p


def refused_reader(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0, late=False):
    """a narrow unit reads the LOAD's image as well (its share waits in buffer 2 and joins the tail as a residual); late: that unit
    stands behind the lead instead of in front of it"""
    p = _prog("leadg_refused_reader" + ("_late" if late else ""), attempt, mmax, cap)
    p.inp("x", 32, dtype, ld=32 + lde)
    p.load("x", 1)
    if not late:
        p.gemm(1, 2, 100, 32, U.NONE)
    p.gemm(1, 0, D, 32, U.RELU)
    if late:
        p.gemm(1, 2, 100, 32, U.NONE)
    src = _run(p, 2, "odd", (U.RELU,), D=D)
    p.gemm(src, 2, 100, D, U.RELU, res=2, ksteps=(D + 15) // 16)
    p.gemm(2, 0, 35, 100, U.NONE, out="y")
    return p


def refused_src(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    """the first run layer takes the buffer that holds the LOAD's image as its SOURCE (a 256-column LOAD filled it before, the 32
    columns lie on top) and adds the lead's output in place: the planner's scan of later readers meets a `src`"""
    p = _prog("leadg_refused_src", attempt, mmax, cap)
    p.inp("r", 256, "bf16", lo=-2, hi=2)
    p.load("r", 1)
    p.inp("x", 32, dtype, ld=32 + lde)
    p.load("x", 1)
    p.gemm(1, 0, D, 32, U.RELU)
    ks = (D + 15) // 16
    p.gemm(1, 0, D, D, U.RELU, res=0, ksteps=ks, nnz=6)
    p.gemm(0, 1, D, D, U.RELU, ksteps=ks, nnz=6)
    p.gemm(1, 0, 35, D, U.NONE, out="y", ksteps=ks)
    return p


def refused_reader_late(lde=0, dtype="bf16", D=256, attempt=0, mmax=U.MMAX, cap=0):
    return refused_reader(lde, dtype, D, attempt, mmax, cap, late=True)


FUSED = {"l32_r2": (l32_r2, 1), "l48_r3": (l48_r3, 1), "l32_r7_leaky": (l32_r7_leaky, 1), "d3": (d3_shaped, 2), "d2": (d2_shaped, 1)}
REFUSED = {"even": refused_even, "store": refused_store, "reader": refused_reader, "src": refused_src}
_CACHE = {}


def get(builder, lde=0, dtype="bf16", D=256):
    """as mlp_unit_util.get: data drawn again from the next seed until the program is exact and not degenerate"""
    key = (builder.__name__, lde, dtype, D)
    if key not in _CACHE:
        for attempt in range(16):
            p = builder(lde, dtype, D, attempt)
            try:
                p.ref()
                U.nondegenerate(p)
                break
            except AssertionError as e:
                if attempt == 15 or not any(m in str(e) for m in ("constant over", "are equal", "must keep it below")):
                    raise
        _CACHE[key] = p
    return _CACHE[key]


# ---- which route does a program get? -------------------------------------------------------------------------------------------
def plans(lib, p, M=300, save_at=None):
    """the planner's word per unit (dhaug_mlp_plan).  Pointers are aligned host memory that nothing dereferences.  save_at: index
    of a GEMM unit that gets a `save` target (forward-with-save)"""
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    ptr = base + (-base) % 16
    units = []
    for i, u in enumerate(p.units):
        m = lib.MlpUnit()
        m.kind, m.src, m.dst, m.res, m.src2 = u["kind"], u.get("src", -1), u.get("dst", -1), u.get("res", -1), u.get("src2", -1)
        if u["kind"] != U.GEMM:
            m.cols, m.ld, m.g = u["cols"], p.tensors[u["t"]]["ld"], ptr
        else:
            m.flags, m.ksteps, m.ksteps2, m.n, m.act, m.slope = u["flags"], u["ksteps"], u["ksteps2"], u["N"], u["act"], u["slope"]
            m.w, m.bias = ptr, ptr
            if u["K2"] or (u["flags"] & U.F_DOT_OUT):
                m.w2 = ptr
            if u["flags"]:
                m.g, m.ld = ptr, p.tensors[u["t"]]["ld"]
            if i == save_at:
                m.save, m.save_ld = ptr, 256
        units.append(m)
    arr = (lib.MlpUnit * len(units))(*units)
    out = (ctypes.c_int32 * len(units))()
    rc = lib.lib().dhaug_mlp_plan(arr, len(units), M, out)
    assert rc == 0, rc
    return list(out)


def fused_places(p, pl):
    """indices of the LOAD units that run as one unit with the stack behind them; checks the word's shape"""
    got = []
    for i, (u, w) in enumerate(zip(p.units, pl)):
        if u["kind"] == U.GEMM or not (w & PLAN_LEADG):
            continue
        assert u["kind"] == U.LOAD_BF16 and (w & PLAN_STACK) and (w & 15) == u["cols"] // 16
        assert (pl[i + 1] & PLAN_STACK) and (pl[i + 1] & 15) == 4 and ((pl[i + 1] >> 4) & 63) == ((w >> 4) & 63)
        got.append(i)
    return got
