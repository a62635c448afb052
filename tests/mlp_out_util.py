"""Programs for the copy-out of dhaug_mlp_forward's outputs (csrc/dhaug_mlp.hip: store_output / store_output_linear, dot_output /
dot_output_once; the shared copy is csrc/dhaug_out_copy.h), built with the harness of tests/mlp_unit_util.py in its exact tier,
and a numpy model of the copy's index arithmetic.

An fp32 output unit (OUT_F32, N <= 64) is reached from two places of the kernel: as the tail of a stack of full-width layers, and
as a single layer.  Its tile leaves as 16-byte groups when the rows are contiguous (ld == N: the planner's PLAN_VSTORE) and by the
rolled dword loop otherwise, or when DHAUG_MLP_NOVSTORE is set."""
import contextlib
import os

import numpy as np

import mlp_unit_util as U

NOVSTORE = "DHAUG_MLP_NOVSTORE"
PLAN_VSTORE, PLAN_OUT = 1 << 8, 1 << 28          # DHAUG_MLP_PLAN_VSTORE of include/dhaug.h; the planner's "fp32 output" bit
MS = (1, 3, 127, 128, 129, 300)
NS = (1, 3, 35, 64)
LD_EXTRA = (0, 5)                                 # ld == N (the new copy) and ld == N + 5 (must keep the loop)
DOT_NS = (20, 40, 70, 100)                        # one, two, three and four waves own a slice of the layer
_CACHE = {}


@contextlib.contextmanager
def vstore(on):
    """the switch of the planner: DHAUG_MLP_NOVSTORE set (any value) keeps the rolled loop"""
    old = os.environ.pop(NOVSTORE, None)
    try:
        if not on:
            os.environ[NOVSTORE] = "1"
        yield
    finally:
        os.environ.pop(NOVSTORE, None)
        if old is not None:
            os.environ[NOVSTORE] = old


def _settle(key, build):
    """like mlp_unit_util.get: the data are drawn again until the exactness condition holds and no output column is degenerate"""
    if key not in _CACHE:
        for attempt in range(16):
            p = build(attempt)
            try:
                p.ref()
                U.nondegenerate(p)
                break
            except AssertionError as e:
                if attempt == 15 or not any(m in str(e) for m in ("constant over", "are equal", "must keep it below")):
                    raise
        _CACHE[key] = p
    return _CACHE[key]


def tail_program(N, lde):
    """two 256 -> 256 layers and a 256 -> N output layer: a stack with the output layer as its tail"""
    name = "out_tail_N%d_ld%d" % (N, lde)

    def build(attempt):
        p = U.Program(name, U._seed(name) + attempt)
        p.inp("x", 256, "f32", lo=-2, hi=2)
        p.load("x", 0)
        p.gemm(0, 1, 256, 256, U.RELU, ksteps=16, nnz=6)
        p.gemm(1, 0, 256, 256, U.RELU, ksteps=16, nnz=6)
        p.gemm(0, 1, N, 256, U.NONE, out="y", ksteps=16, ld=N + lde)
        return p
    return _settle(name, build)


def single_program(N, lde):
    """one K = 64 -> N layer with F_OUT_F32"""
    name = "out_single_N%d_ld%d" % (N, lde)

    def build(attempt):
        p = U.Program(name, U._seed(name) + attempt)
        p.inp("x", 64, "f32")
        p.load("x", 1)
        p.gemm(1, 0, N, 64, U.LRELU, out="y", ld=N + lde)
        return p
    return _settle(name, build)


def dot_program(N, pair=False):
    """a DOT_OUT layer of N features whose scratch buffer (0) was filled with NaN by the unit in front: every partial sum that the
    layer's waves do not write stays NaN.  pair: two narrow layers that run as one unit, the second one the DOT_OUT layer (N > 96)."""
    name = "out_dot_N%d%s" % (N, "_pair" if pair else "")

    def build(attempt):
        p = U.Program(name, U._seed(name) + attempt)
        nan = np.full((p.mmax, 256), np.nan)
        if pair:
            p.inp("nan", 256, "bf16", data=nan)
            p.load("nan", 1)                                                 # (the logits' scratch is buffer 1; x covers columns [0, 128))
            p.inp("x", 104, "f32")
            p.load("x", 1)
            p.gemm(1, 0, 100, 100, U.RELU)
            p.gemm(0, 1, N, 100, U.LRELU, dot="logit")
        else:
            p.inp("nan", 256, "bf16", data=nan)
            p.load("nan", 0)
            p.inp("x", 104, "f32")
            p.load("x", 1)
            p.gemm(1, 0, N, 100, U.RELU, dot="logit")
        return p
    return _settle(name, build)


# ---- the copy's index arithmetic (csrc/dhaug_out_copy.h), in the kernel's 32-bit unsigned integers ------------------------------
OUTC_SHIFT, OUTC_PITCH, OUTC_BM = 19, 68, 128


def outc_magic(N):
    return np.uint32((1 << OUTC_SHIFT) // N + 1)


def outc_row(e, N):
    """row of linear element e as the kernel computes it: (e * magic) >> 19, the product in 32 bits (v_mul_u32_u24: both factors
    must be below 2^24 and the product below 2^32 for the instruction to give the product)"""
    e = np.asarray(e, dtype=np.uint32)
    m = outc_magic(N)
    assert int(m) < 1 << 24 and int(e.max()) < 1 << 24
    assert int(e.max()) * int(m) < 1 << 32
    with np.errstate(over="ignore"):
        return (e * m) >> np.uint32(OUTC_SHIFT)


def outc_lds_byte(e, N):
    """byte offset of element e in the staging image: 4 e + row * 4 (PITCH - N), as the kernel forms it"""
    e = np.asarray(e, dtype=np.uint32)
    skip = np.uint32(4 * (OUTC_PITCH - N))
    row = outc_row(e, N)
    assert int(row.max()) < 1 << 24 and int(row.max()) * int(skip) < 1 << 32
    return np.uint32(4) * e + row * skip


def outc_model(N, rows_live, threads):
    """what one workgroup of `threads` threads writes and reads for a tile with rows_live live rows: (writes, reads) --
    writes: list of (first float offset from out + m0 * N, count, 16-byte store?), reads: staging byte offsets"""
    ng = OUTC_BM * 64 // 4 // threads
    total = rows_live * N
    last = total - 1
    writes, reads = [], []
    for j in range(ng):
        if 4 * threads * j >= total:
            break
        for tid in range(threads):
            e0 = 4 * (tid + threads * j)
            es = np.minimum(np.arange(e0, e0 + 4), last)
            reads.extend(int(b) for b in outc_lds_byte(es, N))
            if e0 + 3 < total:
                writes.append((e0, 4, True))
            else:
                writes.extend((e0 + q, 1, False) for q in range(3) if e0 + q < total)
    return writes, reads
