"""Unit-level harness of dhaug_mlp_forward (csrc/dhaug_mlp.hip): small programs built straight from _lib.MlpUnit, an fp64
reference of the unit semantics, and the exactness check that makes a bit-for-bit comparison legitimate.  Nothing here calls
the kernel under test for a value it is compared with; only Device touches the GPU.

The reference models the three LDS buffers (ids 0, 1: 256 columns; 2: 128) per batch row:
  * LOAD writes columns [0, cols) (fp32 rounded to bf16, round-to-nearest-even) and zeros up to the next multiple of 64;
  * a GEMM unit reads whole 64-column chunks of its sources (4 * ceil(ksteps / 4) k-steps; the packed weights are zero beyond
    K) and writes whole 32-feature slices: columns [0, 32 ceil(N / 32)) -- or all 256 inside a run of full-width layers -- as
    bf16(act(W src [+ W2 src2] + bias + res)), with zero weight rows and zero bias beyond N.  What lies beyond the written
    columns depends on the route the planner takes (a run writes all eight slices, a layer-at-a-time unit leaves the rest as
    it was): the reference marks it "unspecified", and a later unit may only read it under zero weights and only if some
    earlier unit left finite values there (0 * NaN is NaN on the matrix unit as well).  Both are asserted: a program that
    breaks them is a mistake of the test, not of the kernel;
  * OUT_F32 leaves act(.) unrounded in the output tensor; DOT_OUT rounds and activates the features as they would have been
    stored and leaves their dot product with w2 plus the folded bias; both use buffer dst as fp32 scratch, which the
    reference marks undefined;
  * STORE copies columns [0, cols) of a buffer.

Tier 1 (exact): inputs small integers, weights a few nonzeros per row from {+-1/2, +-1}, integer biases, slope 2^-2.  For
every GEMM unit, row and feature the reference asserts sum|terms| < 2^22 q, q the largest power of two dividing every term
(products, bias, residual): then every partial sum in any order is a multiple of q below 2^22 q and fp32 (24 bits) holds it
exactly with two bits to spare, so the kernel's fp32 accumulator holds the exact number whatever its tiling, and the rounding
to bf16 sees the same number as the reference.  Tier 2 (realistic values) is bounded instead: see test_gpu_mlp_units.py."""
import contextlib
import ctypes
import os

import numpy as np

LOAD_F32, LOAD_BF16, STORE_BF16, GEMM = 0, 1, 2, 3
F_OUT_F32, F_DOT_OUT = 4, 16
NONE, RELU, LRELU = 0, 1, 2
PITCH = (256, 256, 128)
MS = (1, 127, 128, 129, 300)                      # the tail tile alone, a ragged tile, a whole tile, one row more, three tiles
MMAX = 300
M_CAP = 128 * 5 + 3                               # six tiles on two workgroups: three each, the ragged one last
EXACT_BITS = 22
NOPAIR, NOTAIL2, NOSTACK = "DHAUG_MLP_NOPAIR", "DHAUG_MLP_NOTAIL2", "DHAUG_MLP_NOSTACK"


# ---- number formats ---------------------------------------------------------------------------------------------------
def bf16_round(a):
    """fp64 values (exactly representable in fp32) -> nearest bf16 value, ties to even, as fp64"""
    f = np.ascontiguousarray(a, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(np.isnan(a), np.nan, out)


def is_bf16(a):
    return bool(np.all(bf16_round(a) == a))


def lowbit(a):
    """largest power of two dividing each (dyadic) value; inf for 0"""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    lb = (mi & -mi).astype(np.float64)
    out = np.ldexp(np.where(lb == 0, 1.0, lb), e - 53)
    return np.where(a == 0, np.inf, out)


def act_fn(v, act, slope):
    if act == RELU:
        return np.maximum(v, 0.0)
    if act == LRELU:
        return np.where(v > 0, v, v * slope)
    return v


def pack_wfrag(W, K=None, k0=0):
    """numpy form of dhaug_pack_wfrag, from the formula in include/dhaug.h:
    dst[((slice*ksteps + ks)*64 + lane)*8 + j] = bf16(W[32 slice + (lane & 31)][k0 + 16 ks + 8 (lane >> 5) + j]), 0 outside
    N x K, ksteps = 4 ceil(K / 64), 8 slices.  Returns the bf16 bit patterns (uint16)."""
    W = np.asarray(W, dtype=np.float64)
    N = W.shape[0]
    K = W.shape[1] - k0 if K is None else K
    ksteps = 4 * ((K + 63) // 64)
    P = np.zeros((256, 16 * ksteps))
    P[:N, :K] = bf16_round(W[:, k0:k0 + K])
    P = P.reshape(8, 32, ksteps, 2, 8).transpose(0, 2, 3, 1, 4)           # (slice, r, ks, h, j) -> (slice, ks, h, r, j)
    f = np.ascontiguousarray(P, dtype=np.float32).reshape(-1)
    return (f.view(np.uint32) >> 16).astype(np.uint16)


def sparse_weights(rng, N, K, nnz):
    """(N, K): nnz nonzeros per row at random columns, values from {+-1/2, +-1}"""
    nnz = min(nnz, K)
    W = np.zeros((N, K))
    idx = np.argsort(rng.random((N, K)), axis=1)[:, :nnz]
    v = rng.choice([-1.0, -0.5, 0.5, 1.0], size=(N, nnz))
    # every row sums to zero (half of its weights are the negatives of the other half): behind ReLU layers the inputs are >= 0 and
    # grow with depth, and a row whose weights lean to the negative side would be dead for every batch row
    h = nnz // 2
    v[:, :h], v[:, h:2 * h] = np.abs(v[:, :h]), -np.abs(v[:, :h])
    W[np.arange(N)[:, None], idx] = v
    return W


# ---- programs ---------------------------------------------------------------------------------------------------------
class Program:
    """a program over named global tensors.  Inputs hold mmax rows; a launch over M rows sees the first M of them, and because
    rows are independent the reference at M is the first M rows of the reference at mmax (computed once, never modified)."""

    def __init__(self, name, seed, mmax=MMAX, env=(), cap=0, tier=1):
        self.name, self.rng, self.mmax, self.env, self.cap, self.tier = name, np.random.default_rng(seed), mmax, tuple(env), cap, tier
        self.units, self.tensors = [], {}
        self._ref = None

    # global tensors: dict(dtype "f32" | "bf16", width, ld, data (inputs) | None, ncheck)
    def inp(self, name, width, dtype="f32", ld=None, lo=-4, hi=4, data=None):
        ld = width + 8 if ld is None else ld
        if data is None:
            data = self.rng.integers(lo, hi + 1, size=(self.mmax, width)).astype(np.float64)
        data = np.asarray(data, dtype=np.float64).astype(np.float32).astype(np.float64)
        if dtype == "bf16":
            data = bf16_round(data)
        self.tensors[name] = dict(dtype=dtype, width=width, ld=ld, data=data, ncheck=0)
        return name

    def _out(self, name, width, dtype, ld, ncheck):
        assert name not in self.tensors
        self.tensors[name] = dict(dtype=dtype, width=width, ld=width + 8 if ld is None else ld, data=None, ncheck=ncheck)

    def load(self, t, dst, cols=None):
        T = self.tensors[t]
        self.units.append(dict(kind=LOAD_BF16 if T["dtype"] == "bf16" else LOAD_F32, t=t, dst=dst,
                               cols=T["width"] if cols is None else cols))

    def store(self, src, cols, t, ld=None, ncheck=None):
        self._out(t, cols, "bf16", ld, cols if ncheck is None else ncheck)
        self.units.append(dict(kind=STORE_BF16, t=t, src=src, cols=cols))

    def gemm(self, src, dst, N, K, act=NONE, slope=0.25, res=-1, src2=-1, K2=0, out=None, dot=None, ksteps=None, ksteps2=None,
             nnz=8, W=None, b=None, ld=None, real=False, composed=None):
        """K (+ K2) true input columns.  out: name of the fp32 tensor of an OUT_F32 unit; dot: name of the logit tensor of a
        DOT_OUT unit.  real (tier 2): normal weights / sqrt(K), biases that are no bf16 values.  composed = (Wa, ba, Wb, bb):
        the unit's weights are the composite of two layers (dhaug_pack_wfrag_composed)."""
        rng = self.rng
        if W is None:
            if real:
                W = bf16_round((rng.standard_normal((N, K + K2)) / np.sqrt(K + K2)).astype(np.float32).astype(np.float64))
            else:
                W = sparse_weights(rng, N, K + K2, nnz if N >= 8 else 32)
        if b is None:
            if real:
                b = (0.1 * rng.standard_normal(N)).astype(np.float32).astype(np.float64) + 0.1 + 2.0 ** -13
                b = b.astype(np.float32).astype(np.float64)
            else:
                b = rng.integers(-1 if act == RELU else -2, 4 if act == RELU else 3, size=N).astype(np.float64)   # (fewer dead columns)
        u = dict(kind=GEMM, src=src, dst=dst, res=res, src2=src2, N=N, K=K, K2=K2, act=act, slope=slope, W=W, b=b, flags=0,
                 ksteps=(K + 15) // 16 if ksteps is None else ksteps, real=real, composed=composed,
                 ksteps2=0 if K2 == 0 else ((K2 + 15) // 16 if ksteps2 is None else ksteps2))
        if out is not None:
            u["flags"], u["t"] = F_OUT_F32, out
            self._out(out, N, "f32", ld, N)
        if dot is not None:
            u["flags"], u["t"] = F_DOT_OUT, dot
            if real:
                u["dotw"] = bf16_round((rng.standard_normal(N) / np.sqrt(N)).astype(np.float32).astype(np.float64))
                u["dotb"] = float(np.float32(0.1 + 2.0 ** -13))
            else:
                u["dotw"] = rng.choice([-1.0, -0.5, 0.5, 1.0], size=N)
                u["dotb"] = float(rng.integers(-2, 3))
            self._out(dot, 1, "f32", 3 if ld is None else ld, 1)
        self.units.append(u)
        return u

    def ref(self):
        if self._ref is None:
            self._ref = reference(self)
        return self._ref


class _State:
    def __init__(self, M):
        self.val = [np.full((M, p), np.nan) for p in PITCH]
        self.spec = [np.zeros(p, dtype=bool) for p in PITCH]
        self.bnd = [np.zeros((M, p)) for p in PITCH]                       # tier 2: error bound of each value

    def read(self, b, ncols, Wp, what):
        """columns [0, ncols) of buffer b as a GEMM operand against the zero-padded weights Wp (rows x ncols)"""
        v, s = self.val[b][:, :ncols], self.spec[b][:ncols]
        assert not np.isnan(v).any(), "%s: reads columns of buffer %d that no unit has written" % (what, b)
        assert not Wp[:, ~s].any(), "%s: nonzero weights on columns of buffer %d whose content depends on the route" % (what, b)
        return np.where(s[None, :], v, 0.0)

    def undefine(self, b):
        self.val[b][:] = np.nan
        self.spec[b][:] = False
        self.bnd[b][:] = 0.0


def _exactness(what, x, W, extra, fmt=None, fmt_name="bf16"):
    """asserts the condition of the module docstring for pre = x W^T + sum(extra) and returns the bits it needs.  x (M, K),
    W (N, K), extra: list of (M, N) or (N,) arrays (bias, residual).  fmt: the predicate the operands must satisfy (default:
    bf16 values; the parity harness, tests/mlp_x3_unit_util.py, passes fp16 pieces)."""
    fmt = is_bf16 if fmt is None else fmt
    assert fmt(x) and fmt(W), "%s: an operand is no %s value" % (what, fmt_name)
    S = np.abs(x) @ np.abs(W).T
    nz = W != 0
    nnz = int(nz.sum(1).max()) if W.size else 0
    if 0 < nnz <= 40:                                                       # exact q of the products, per row and feature
        order = np.argsort(~nz, axis=1, kind="stable")[:, :nnz]             # the nonzero columns of each feature first
        valid = np.take_along_axis(nz, order, 1)
        lbw = np.where(valid, lowbit(np.take_along_axis(W, order, 1)), np.inf)
        lbx = lowbit(x)
        q = np.min(lbx[:, order] * lbw[None, :, :], axis=2)                # (M, N)
    else:                                                                   # dense weights: a lower bound of q
        lbx = lowbit(x).min(axis=1) if x.size else np.array([np.inf])
        lbw = np.where(nz, lowbit(W), np.inf).min(axis=1) if W.size else np.array([np.inf])
        q = lbx[:, None] * lbw[None, :]
    for e in extra:
        e2 = np.broadcast_to(e, S.shape)
        S = S + np.abs(e2)
        q = np.minimum(q, lowbit(e2))
    live = np.isfinite(q)                                                   # (a sum with no nonzero term is exact)
    if not live.any():
        return 0.0
    need = np.log2(np.where(live, S, 1.0) / np.where(live, q, 1.0))
    worst = float(need.max())
    assert worst < EXACT_BITS, "%s: sum|terms| / q = 2^%.1f, the data must keep it below 2^%d" % (what, worst, EXACT_BITS)
    return worst


def composed_weights(Wa, ba, Wb, bb):
    """the documented rule of dhaug_pack_wfrag_composed: sums in fp64, rounded to fp32, weights then once to bf16"""
    W = bf16_round((Wa @ Wb).astype(np.float32).astype(np.float64))
    b = (Wa @ bb + ba).astype(np.float32).astype(np.float64)
    return W, b


def reference(p):
    """fp64 evaluation of the program over its mmax rows -> dict(out: name -> (mmax, width) values, bound: name -> error bounds
    (tier 2; zeros in tier 1), bits: the largest log2(sum|terms| / q) of the program)"""
    M = p.mmax
    st = _State(M)
    out, bound, bits = {}, {}, 0.0
    # whether a unit runs alone, in a pair or in a run of full-width layers does not matter for the columns [0, 32 ceil(N/32)): the
    # same formula on every route; the columns beyond are "unspecified" whatever the route
    for i, u in enumerate(p.units):
        what = "%s unit %d" % (p.name, i)
        k = u["kind"]
        if k in (LOAD_F32, LOAD_BF16):
            T, cols, b = p.tensors[u["t"]], u["cols"], u["dst"]
            assert cols % 8 == 0 and cols <= T["width"] and ((cols + 63) & ~63) <= PITCH[b]
            data = T["data"] if T["data"] is not None else out[u["t"]]      # (a parked tensor: what the STORE left)
            pad = (cols + 63) & ~63
            st.val[b][:, :cols] = bf16_round(data[:, :cols])
            st.val[b][:, cols:pad] = 0.0
            st.spec[b][:pad] = True
            st.bnd[b][:, :pad] = 0.0 if T["data"] is not None else np.pad(bound[u["t"]][:, :cols], ((0, 0), (0, pad - cols)))
        elif k == STORE_BF16:
            b, cols = u["src"], u["cols"]
            assert cols % 8 == 0 and st.spec[b][:cols].all() and not np.isnan(st.val[b][:, :cols]).any(), what + ": stores undefined columns"
            out[u["t"]] = st.val[b][:, :cols].copy()
            bound[u["t"]] = st.bnd[b][:, :cols].copy()
        else:
            N, K, K2 = u["N"], u["K"], u["K2"]
            W, bias = u["W"], u["b"]
            if u["composed"] is not None:
                W, bias = composed_weights(*u["composed"])
            Np = 32 * ((N + 31) // 32)
            kp1, kp2 = 64 * ((u["ksteps"] + 3) // 4), 64 * ((u["ksteps2"] + 3) // 4)
            assert K <= 16 * u["ksteps"] and K2 <= 16 * u["ksteps2"] and kp1 <= PITCH[u["src"]]
            W1 = np.zeros((Np, kp1)); W1[:N, :K] = W[:, :K]
            x = st.read(u["src"], kp1, W1, what)
            xb = st.bnd[u["src"]][:, :kp1]
            Wc = W1
            if K2:
                W2 = np.zeros((Np, kp2)); W2[:N, :K2] = W[:, K:K + K2]
                x = np.concatenate([x, st.read(u["src2"], kp2, W2, what)], axis=1)
                xb = np.concatenate([xb, st.bnd[u["src2"]][:, :kp2]], axis=1)
                Wc = np.concatenate([W1, W2], axis=1)
            bp = np.zeros(Np); bp[:N] = bias
            extra, rspec = [bp], np.ones(Np, dtype=bool)
            to_global = bool(u["flags"] & F_OUT_F32)
            if u["res"] >= 0:
                assert not to_global, what + ": an OUT_F32 unit takes no residual"
                r = st.val[u["res"]][:, :Np]
                rspec = st.spec[u["res"]][:Np].copy()
                assert not np.isnan(r).any() and rspec[:N].all(), what + ": residual columns undefined"
                extra.append(np.where(rspec[None, :], r, 0.0))
            pre = x @ Wc.T
            for e in extra:
                pre = pre + e
            if u["real"]:
                assert not xb.any() and (u["res"] < 0 or not st.bnd[u["res"]][:, :Np].any()), what + ": tier 2 input is not exactly known"
                S = np.abs(x) @ np.abs(Wc).T
                for e in extra:
                    S = S + np.abs(e)
                eb = (K + K2 + 2) * 2.0 ** -24 * S
            else:
                bits = max(bits, _exactness(what, x, Wc, extra))
                assert (pre.astype(np.float32).astype(np.float64) == pre).all()
                eb = np.zeros_like(pre)
            y = act_fn(pre, u["act"], u["slope"])
            if to_global:
                out[u["t"]], bound[u["t"]] = y[:, :N].copy(), eb[:, :N].copy()   # |act(a) - act(b)| <= |a - b|
                st.undefine(u["dst"])
            elif u["flags"] & F_DOT_OUT:
                w2 = np.zeros(Np); w2[:N] = u["dotw"]
                assert is_bf16(w2)
                a = bf16_round(y)
                if u["real"]:
                    # the kernel's activation lies between the roundings of act(pre -+ eb): the rounding may fall the other way
                    lo, hi = bf16_round_any(act_fn(pre - eb, u["act"], u["slope"])), bf16_round_any(act_fn(pre + eb, u["act"], u["slope"]))
                    amax = np.maximum(np.abs(lo), np.abs(hi))
                    S2 = amax @ np.abs(w2) + abs(u["dotb"])
                    bound[u["t"]] = ((hi - lo) @ np.abs(w2) + 130 * 2.0 ** -24 * S2)[:, None]
                else:
                    bits = max(bits, _exactness(what + " (dot)", a, w2[None, :], [np.full((1,), u["dotb"])]))
                    bound[u["t"]] = np.zeros((M, 1))
                out[u["t"]] = (a @ w2 + u["dotb"])[:, None]
                st.undefine(u["dst"])
            else:
                d = u["dst"]
                assert Np <= PITCH[d]
                # (tier 2: the fp64 value itself; the kernel's rounding to bf16 is the 2^-8 |ref| of the bound)
                st.val[d][:, :Np] = y if u["real"] else bf16_round(y)
                st.bnd[d][:, :Np] = eb + (2.0 ** -8 * np.abs(y) if u["real"] else 0.0)
                st.spec[d][:Np] = rspec
                st.spec[d][Np:] = False                                     # a run writes them, a single layer does not
    return dict(out=out, bound=bound, bits=bits)


def bf16_round_any(a):
    """bf16_round for values that need not be fp32 values (tier 2): the nearest fp32 first"""
    return bf16_round(np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64))


def nondegenerate(p):
    """every checked output column differs between two rows and no two of them are equal: a swapped row, column or chunk shows"""
    r = p.ref()
    for name, T in p.tensors.items():
        if T["data"] is not None or name not in r["out"]:
            continue
        v = r["out"][name][:, :T["ncheck"]]
        assert np.isfinite(v).all(), (p.name, name)
        assert (v.max(axis=0) != v.min(axis=0)).all(), "%s: a column of %s is constant over the rows" % (p.name, name)
        assert np.unique(v, axis=1).shape[1] == v.shape[1], "%s: two columns of %s are equal" % (p.name, name)


# ---- the program families ---------------------------------------------------------------------------------------------
REG = {}                                          # name -> (family, builder)
_CACHE = {}


def _reg(family, name):
    def deco(fn):
        assert name not in REG
        REG[name] = (family, fn)
        return fn
    return deco


def get(name):
    """the program of that name.  Its random data are drawn again, from the next seed, until the exactness condition holds and the
    outputs are not degenerate (a ReLU column that is dead for every row, two equal weight rows): deterministic, and what comes
    back is asserted once more by tests/test_mlp_units_cpu.py.  A program whose STRUCTURE is wrong fails at once."""
    if name not in _CACHE:
        for attempt in range(16):
            p = REG[name][1](attempt)
            try:
                p.ref()
                nondegenerate(p)
                break
            except AssertionError as e:
                if attempt == 15 or not any(m in str(e) for m in ("constant over", "are equal", "must keep it below")):
                    raise
        _CACHE[name] = p
    return _CACHE[name]


def names(family):
    return [n for n, (f, _) in REG.items() if f == family]


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 63)


def _load_pad(cols):
    return (cols + 7) & ~7


# 1. single layer-at-a-time units
K1 = (8, 48, 64, 72, 128, 200, 256)
N1 = (1, 31, 32, 33, 64, 100, 128, 129, 224, 225, 256)
_ACTS = (NONE, RELU, LRELU)


def _single(name, K, N, act, resmode, src, dst, out_f32, in_dtype="f32", ld_extra=8, big=False, mmax=MMAX, cap=0):
    """LOAD -> GEMM -> OUT_F32 | STORE.  resmode 0: none, 1: in place (res == dst), 2: from the third buffer"""
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt, mmax=mmax, cap=cap)
        third = 3 - src - dst
        Np = 32 * ((N + 31) // 32)
        cols = _load_pad(K)
        # fp32 inputs that are no bf16 values (|x| up to 300): the LOAD's rounding is part of the reference
        p.inp("x", cols, in_dtype, ld=cols + ld_extra, lo=-300 if big else -4, hi=300 if big else 4)
        if cols > K:
            p.tensors["x"]["data"][:, K:] = 7.0                              # finite, under zero weights
        p.load("x", src)
        res = -1
        if resmode:
            res = dst if resmode == 1 else third
            p.inp("r", Np, "bf16" if in_dtype == "f32" else "f32", lo=-6, hi=6)
            p.load("r", res)
        if out_f32:
            p.gemm(src, dst, N, K, act, res=res, out="y")
        else:
            p.gemm(src, dst, N, K, act, res=res)
            p.store(dst, _load_pad(N), "y", ncheck=N)
        return p
    return build


def _register_singles():
    i = 0
    for iK, K in enumerate(K1):
        for iN, N in enumerate(N1):
            # every activation and every residual form meets every K and every N, and all nine pairs occur
            act, resmode = _ACTS[(iK + iN) % 3], (iK + 2 * iN) % 3
            out_f32 = N <= 64 and ((iK + iN) % 2 == 0)
            if out_f32:
                resmode = 0                                                  # (an OUT_F32 unit takes no residual)
            Np = 32 * ((N + 31) // 32)
            if resmode == 2 and K > 128 and Np > 128:
                resmode = 1                                                  # (no third buffer that wide: source and result take 0 and 1)
            pairs = [(s, d) for s, d in ((1, 0), (0, 1), (2, 0), (0, 2), (2, 1), (1, 2))
                     if (s != 2 or K <= 128) and (d != 2 or (Np <= 128 and not out_f32))
                     and (resmode != 2 or 3 - s - d != 2 or Np <= 128)]
            src, dst = pairs[i % len(pairs)]
            name = "single_K%d_N%d_a%d_r%d_s%dd%d_%s" % (K, N, act, resmode, src, dst, "f32" if out_f32 else "st")
            in_dtype = "bf16" if i % 4 == 1 else "f32"
            _reg("single", name)(_single(name, K, N, act, resmode, src, dst, out_f32, in_dtype, ld_extra=0 if i % 5 == 0 else 8,
                                         big=(i % 4 == 2)))
            i += 1
    # every N <= 64 both as an fp32 output and through a STORE; buffer 2 on both sides; the contiguous-row LOAD forms
    extra = [(64, 1, RELU, 2, 1, 0, False, "f32", 0), (128, 31, LRELU, 1, 2, 1, False, "bf16", 8), (48, 32, NONE, 0, 1, 0, True, "f32", 0),
             (48, 33, LRELU, 2, 0, 1, False, "f32", 0), (128, 64, RELU, 0, 2, 0, True, "f32", 0), (32, 64, LRELU, 0, 1, 0, True, "f32", 0),
             (32, 128, RELU, 1, 1, 2, False, "bf16", 0), (16, 100, NONE, 2, 0, 2, False, "f32", 0), (128, 128, LRELU, 2, 2, 0, False, "f32", 8),
             (256, 1, NONE, 0, 0, 1, True, "bf16", 8), (200, 33, RELU, 0, 1, 0, True, "f32", 8), (72, 256, LRELU, 2, 2, 0, False, "bf16", 8)]
    for K, N, act, resmode, src, dst, out_f32, in_dtype, lde in extra:
        name = "single_x_K%d_N%d_a%d_r%d_s%dd%d_%s_%s%d" % (K, N, act, resmode, src, dst, "f32" if out_f32 else "st", in_dtype, lde)
        _reg("single", name)(_single(name, K, N, act, resmode, src, dst, out_f32, in_dtype, lde))
    name = "single_cap"
    _reg("cap", name)(_single(name, 200, 225, LRELU, 1, 0, 1, False, "f32", 8, mmax=M_CAP, cap=2))


# 2. two-source units
def _two_source(name, K, K2, N, src, src2, dst, act, res=-1, kcols2=None, mmax=MMAX, cap=0):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt, mmax=mmax, cap=cap)
        c2 = K2 if kcols2 is None else kcols2
        p.inp("a", K, "f32")
        p.inp("b", c2, "bf16")
        p.load("a", src)
        p.load("b", src2)
        if res >= 0:
            p.inp("r", 32 * ((N + 31) // 32), "bf16", lo=-6, hi=6)
            p.load("r", res)
        # (K2 true columns; the unit is handed the k-steps of the columns loaded, the weights beyond K2 are zero)
        p.gemm(src, dst, N, K, act, res=res, src2=src2, K2=K2, ksteps2=(c2 + 15) // 16)
        p.store(dst, _load_pad(N), "y", ncheck=N)
        return p
    return build


def _register_two_source():
    cases = [("two_33_n100", 64, 64, 100, 0, 1, 2, RELU, -1, None), ("two_33_n256", 64, 64, 256, 2, 0, 1, LRELU, 1, None),
             ("two_33_n33", 64, 64, 33, 1, 2, 0, NONE, -1, None),
             ("two_66_n128", 128, 128, 128, 0, 1, 2, LRELU, 2, None), ("two_66_n256", 128, 128, 256, 2, 1, 0, RELU, -1, None),
             # 128 + 40: the second source is loaded 128 wide (two chunks, the layout of shape 66) and carries 40 weight columns
             ("two_66_k40", 128, 40, 100, 1, 0, 2, RELU, -1, 128), ("two_66_k40_n225", 128, 40, 225, 2, 0, 1, NONE, -1, 128),
             ("two_132_n128", 256, 256, 128, 0, 1, 2, RELU, -1, None), ("two_132_n100", 256, 256, 100, 1, 0, 2, LRELU, 2, None),
             ("two_132_n1", 256, 256, 1, 0, 1, 2, NONE, -1, None)]
    for name, K, K2, N, s, s2, d, act, res, kc in cases:
        _reg("two", name)(_two_source(name, K, K2, N, s, s2, d, act, res, kc))
    _reg("cap", "two_cap")(_two_source("two_cap", 256, 256, 100, 0, 1, 2, LRELU, 2, None, mmax=M_CAP, cap=2))


# 3. narrow layers (K 65..128, N 97..128): pairs
def _narrow(name, widths, res_second=False, dot_last=False, env=(), mmax=MMAX, cap=0):
    """LOAD K0 -> buffer 1, then layers of the given widths alternating between buffers 0 and 1"""
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt, mmax=mmax, env=env, cap=cap)
        K = widths[0]
        p.inp("x", _load_pad(K), "f32")
        p.load("x", 1)
        if res_second:
            p.inp("r", 128, "bf16", lo=-6, hi=6)
            p.load("r", 2)
        src = 1
        acts = (RELU, LRELU, NONE, RELU)
        for j, N in enumerate(widths[1:]):
            last = j == len(widths) - 2
            res = 2 if (res_second and j == 1) else -1
            if last and dot_last:
                p.gemm(src, 1 - src, N, K, acts[j], res=res, dot="logit")
            else:
                p.gemm(src, 1 - src, N, K, acts[j], res=res)
            src, K = 1 - src, N
        if not dot_last:
            p.store(src, _load_pad(K), "y", ncheck=K)
        return p
    return build


def _dot_single(name, K, N, act, ld):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt)
        p.inp("x", _load_pad(K), "bf16")
        p.load("x", 1)
        p.gemm(1, 0, N, K, act, dot="logit", ld=ld)
        return p
    return build


def _register_narrow():
    cases = [("narrow2", (100, 100, 128), {}), ("narrow3", (72, 97, 128, 100), {}), ("narrow4", (128, 100, 97, 128, 112), {}),
             ("narrow2_res", (100, 128, 100), dict(res_second=True)), ("narrow2_dot", (80, 100, 100), dict(dot_last=True)),
             ("narrow4_res_dot", (100, 100, 128, 100, 97), dict(res_second=True, dot_last=True))]
    for name, widths, kw in cases:
        _reg("narrow", name)(_narrow(name, widths, **kw))
        _reg("narrow", name + "_nopair")(_narrow(name + "_nopair", widths, env=(NOPAIR,), **kw))
    for K, N, act, ld in ((100, 1, NONE, 2), (128, 64, RELU, 3), (72, 128, LRELU, 5), (64, 128, RELU, 2)):
        name = "dot_K%d_N%d" % (K, N)
        _reg("narrow", name)(_dot_single(name, K, N, act, ld))
    _reg("cap", "narrow_cap")(_narrow("narrow_cap", (100, 100, 128, 100, 97), res_second=True, dot_last=True, mmax=M_CAP, cap=2))


# 4. stacks
def _stack(name, lead, run, respat, acts, tail, widths=None, env=(), mmax=MMAX, cap=0):
    """lead: K of the narrow lead layer, or None (the first run layer reads a 256-column LOAD).  respat: "none" | "odd" | "even"
    (positions of the run that carry an in-place residual).  acts: activation of run layer j = acts[j % len(acts)].  widths:
    {run position: N} for layers narrower than 256 (their consumer still gets ksteps = 16).  tail: None (STORE) |
    ("f32", N) | ("bf16", N, dst, res)"""
    widths = widths or {}

    def build(attempt=0):
        p = Program(name, _seed(name) + attempt, mmax=mmax, env=env, cap=cap)
        # the run alternates between buffers 0 and 1; a residual is in place (res == dst), so the buffer a run layer adds to must
        # be whole before the run: a 256-column LOAD first, the lead layer's input on top of it where both use the same buffer
        if lead is None:
            first_src = 0
            if respat == "even":
                p.inp("r", 256, "bf16", lo=-3, hi=3)
                p.load("r", 1)
            p.inp("x", 256, "f32", lo=-2, hi=2)
            p.load("x", 0)
        else:
            first_src = 0
            if respat == "even":
                p.inp("r", 256, "bf16", lo=-3, hi=3)
                p.load("r", 1)
            p.inp("x", lead, "f32", ld=lead if lead in (32, 48, 128) and (run % 2) else None)
            p.load("x", 1)
            p.gemm(1, 0, 256, lead, acts[0])
        src, K = first_src, 256
        for j in range(run):
            N = widths.get(j, 256)
            has_res = (respat == "odd" and j % 2 == 1) or (respat == "even" and j % 2 == 0)
            p.gemm(src, 1 - src, N, K, acts[j % len(acts)], res=(1 - src) if has_res else -1, ksteps=16, nnz=6)
            src, K = 1 - src, N
        if tail is None:
            p.store(src, _load_pad(K), "y", ncheck=K)
        elif tail[0] == "f32":
            p.gemm(src, 1 - src, tail[1], K, NONE, out="y", ksteps=16)
        else:
            _, N, dst, res = tail
            if res == 2:
                p.inp("r2", 128, "bf16", lo=-6, hi=6)
                p.load("r2", 2)
            p.gemm(src, dst, N, K, RELU, res=res, ksteps=16)
            p.store(dst, _load_pad(N), "y", ncheck=N)
        return p
    return build


def _register_stacks():
    R, L, X = (RELU,), (LRELU,), (NONE,)
    cases = [
        # name, lead, run, residuals, activations, tail, widths
        ("stack_gen", 128, 6, "odd", R, ("f32", 35), None),                    # the generator's shape: PLAN_ALT
        ("stack_l32_r2_none", 32, 2, "none", R, None, None),
        ("stack_l48_r3_odd", 48, 3, "odd", R, ("f32", 1), None),
        ("stack_nolead_r2_odd", None, 2, "odd", R, ("f32", 64), None),        # PLAN_ALT without a lead
        ("stack_nolead_r7_even", None, 7, "even", R, None, None),
        ("stack_l128_r6_even", 128, 6, "even", (RELU, RELU, NONE), ("bf16", 100, 2, -1), None),
        ("stack_l32_r7_odd_leaky", 32, 7, "odd", L, ("bf16", 128, 2, 2), None),
        ("stack_nolead_r3_mixed", None, 3, "none", (RELU, LRELU), ("bf16", 100, 0, -1), None),   # the tail's dst is the buffer left
        ("stack_l48_r6_odd_plain", 48, 6, "odd", (RELU, RELU, RELU, NONE), None, None),           # ALT with an activation-free layer
        ("stack_l128_r2_n232", 128, 2, "odd", R, ("f32", 35), {0: 232}),
        ("stack_nolead_r3_n225", None, 3, "none", L, None, {1: 225}),
        ("stack_l32_r6_n232_n225", 32, 6, "odd", R, ("bf16", 128, 2, -1), {2: 232, 3: 225}),
        ("stack_nolead_r2_leaky_f32", None, 2, "even", L, ("f32", 35), None),
        ("stack_l128_r3_none_plain", 128, 3, "none", X + R, ("bf16", 128, 2, 2), None),
    ]
    for name, lead, run, respat, acts, tail, widths in cases:
        _reg("stack", name)(_stack(name, lead, run, respat, acts, tail, widths))
        if tail is not None and tail[0] == "bf16":
            _reg("stack", name + "_notail2")(_stack(name + "_notail2", lead, run, respat, acts, tail, widths, env=(NOTAIL2,)))
    for name in ("stack_gen", "stack_l32_r7_odd_leaky"):
        lead, run, respat, acts, tail, widths = [c[1:] for c in cases if c[0] == name][0]
        _reg("stack", name + "_nostack")(_stack(name + "_nostack", lead, run, respat, acts, tail, widths, env=(NOSTACK,)))
    _reg("cap", "stack_cap")(_stack("stack_cap", 128, 6, "odd", R, ("f32", 35), None, mmax=M_CAP, cap=2))
    _reg("cap", "stack_cap_bf16")(_stack("stack_cap_bf16", None, 3, "even", L, ("bf16", 100, 2, 2), {1: 232}, mmax=M_CAP, cap=2))


# 5. parking, 6. stale columns
def _parking(name, mmax=MMAX, cap=0):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt, mmax=mmax, cap=cap)
        p.inp("x", 64, "f32")
        p.load("x", 1)
        p.gemm(1, 0, 256, 64, RELU)
        p.store(0, 256, "park", ld=264)                                      # parked: global memory, bf16
        p.gemm(0, 1, 128, 256, LRELU)
        p.gemm(1, 0, 256, 128, RELU)                                         # buffer 0 is overwritten
        p.gemm(0, 2, 100, 256, NONE)
        p.load("park", 1)                                                    # LOAD_BF16 of the parked rows (behind the drain barrier)
        p.gemm(1, 0, 128, 256, RELU, res=2)                                  # ... as a source
        p.gemm(0, 2, 128, 128, LRELU)
        p.gemm(2, 0, 256, 128, NONE, res=1)                                  # ... and as a residual
        p.store(0, 256, "y")
        return p
    return build


def _stale(name, mmax=MMAX, cap=0):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt, mmax=mmax, cap=cap)
        p.inp("x", 64, "f32")
        p.load("x", 1)
        big = (p.rng.integers(1, 64, size=256) * 512.0) * p.rng.choice([-1.0, 1.0], size=256)
        p.gemm(1, 0, 256, 64, NONE, b=big)                                   # large finite values in all 256 columns
        p.gemm(1, 0, 72, 64, RELU)                                           # columns [0, 96) rewritten, the rest stale
        p.gemm(0, 1, 128, 72, LRELU)                                         # reads [0, 128): zero weights beyond 72
        p.store(1, 128, "y")
        return p
    return build


def _register_rest():
    _reg("park", "parking")(_parking("parking"))
    _reg("cap", "parking_cap")(_parking("parking_cap", mmax=M_CAP, cap=2))
    _reg("stale", "stale_columns")(_stale("stale_columns"))
    _reg("cap", "stale_cap")(_stale("stale_cap", mmax=M_CAP, cap=2))


# tier 2: one unit per shape class with realistic values (M = 129)
def _real(name, kind):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt, mmax=129, tier=2)
        rng = p.rng
        normal = lambda w: rng.standard_normal((p.mmax, w))
        if kind in ("17", "34", "68"):
            K = {"17": 48, "34": 100, "68": 256}[kind]
            p.inp("x", _load_pad(K), "f32", data=normal(_load_pad(K)))
            p.load("x", 1)
            p.inp("r", 256, "bf16", data=normal(256))
            p.load("r", 0)
            p.gemm(1, 0, 256, K, LRELU, slope=0.01, res=0, real=True)
            p.store(0, 256, "y")
        elif kind == "68_f32":
            p.inp("x", 256, "bf16", data=normal(256))
            p.load("x", 0)
            p.gemm(0, 1, 35, 256, LRELU, slope=0.01, real=True, out="y")
        elif kind in ("33", "66", "132"):
            K = {"33": 64, "66": 128, "132": 256}[kind]
            p.inp("a", K, "f32", data=normal(K))
            p.inp("b", K, "bf16", data=normal(K))
            p.load("a", 0)
            p.load("b", 1)
            p.gemm(0, 2, 100, K, LRELU, slope=0.01, src2=1, K2=K, real=True)
            p.store(2, 104, "y", ncheck=100)
        elif kind == "stack":                                                # an exact first layer, then the realistic one
            p.inp("x", 256, "f32", lo=-2, hi=2)
            p.load("x", 0)
            p.gemm(0, 1, 256, 256, RELU, ksteps=16, nnz=6)
            p.gemm(1, 0, 256, 256, LRELU, slope=0.01, real=True)
            p.store(0, 256, "y")
        elif kind == "stack_tail":
            p.inp("x", 256, "f32", lo=-2, hi=2)
            p.load("x", 0)
            p.gemm(0, 1, 256, 256, RELU, ksteps=16, nnz=6)
            p.gemm(1, 0, 256, 256, RELU, ksteps=16, nnz=6)
            p.gemm(0, 1, 35, 256, NONE, real=True, out="y")
        elif kind == "pair":
            p.inp("x", 104, "f32")
            p.load("x", 1)
            p.gemm(1, 0, 100, 100, RELU)
            p.gemm(0, 1, 100, 100, LRELU, slope=0.01, real=True)
            p.store(1, 104, "y", ncheck=100)
        elif kind == "dot":
            p.inp("x", 104, "f32", data=normal(104))
            p.load("x", 1)
            p.gemm(1, 0, 100, 100, LRELU, slope=0.01, real=True, dot="logit")
        elif kind == "pair_dot":
            p.inp("x", 104, "f32")
            p.load("x", 1)
            p.gemm(1, 0, 100, 100, RELU)
            p.gemm(0, 1, 100, 100, RELU, real=True, dot="logit")
        return p
    return build


def _register_real():
    for kind in ("17", "34", "68", "68_f32", "33", "66", "132", "stack", "stack_tail", "pair", "dot", "pair_dot"):
        _reg("real", "real_" + kind)(_real("real_" + kind, kind))


# 7. the shipped builders: the programs of fused.py (GEN, D2 with its composed layer, D3) written out unit by unit, with the
# parameters kept as a state_dict (p.sd) that the GPU test loads into the modules before it calls fused.generator_head /
# critic2d / critic3d
def _ship_gen(name, D):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt)
        p.sd = {}

        def lin(key, *a, **kw):
            u = p.gemm(*a, **kw)
            p.sd[key + ".weight"], p.sd[key + ".bias"] = u["W"], u["b"]

        p.inp("z", 128, "f32", ld=128)
        p.load("z", 1)
        lin("preprocess.0", 1, 0, D, 128, RELU)
        for b in ("block1", "block2", "block3"):
            lin(b + ".fc1", 0, 1, D, D, RELU, nnz=6)
            lin(b + ".fc2", 1, 0, D, D, RELU, res=0, nnz=6)
        lin("deconv_out", 0, 1, 35, D, NONE, out="y")
        return p
    return build


def _ship_d2(name, D):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt)
        p.sd = {}

        def lin(key, *a, **kw):
            u = p.gemm(*a, **kw)
            p.sd[key + ".weight"], p.sd[key + ".bias"] = u["W"], u["b"]

        p.inp("x", 32, "f32", ld=32)
        p.load("x", 1)
        lin("pose_layer_1", 1, 0, D, 32, LRELU)
        lin("pose_layer_2", 0, 1, D, D, LRELU, nnz=6)
        lin("pose_layer_3", 1, 0, D, D, LRELU, res=0, nnz=6)
        # pose_layer_4 (no activation) and layer_last as one layer: W_last W_4, W_last b_4 + b_last
        Wb, bb = sparse_weights(p.rng, D, D, 4), p.rng.integers(-2, 3, size=D).astype(np.float64)
        Wa, ba = sparse_weights(p.rng, D, D, 4), p.rng.integers(-2, 3, size=D).astype(np.float64)
        W, b = composed_weights(Wa, ba, Wb, bb)
        assert np.array_equal(W, Wa @ Wb)                                    # (the composite of these factors needs no rounding)
        p.gemm(0, 1, D, D, LRELU, W=W, b=b, composed=(Wa, ba, Wb, bb))
        p.sd.update({"pose_layer_4.weight": Wb, "pose_layer_4.bias": bb, "layer_last.weight": Wa, "layer_last.bias": ba})
        lin("layer_pred", 1, 0, 1, D, NONE, out="y")
        return p
    return build


def _ship_d3(name, D):
    def build(attempt=0):
        p = Program(name, _seed(name) + attempt)
        p.sd = {}

        def lin(key, *a, **kw):
            u = p.gemm(*a, **kw)
            p.sd[key + ".weight"], p.sd[key + ".bias"] = u["W"], u["b"]
            return u

        def blocks(names_):
            for b in names_:
                lin(b + ".fc1", 0, 1, D, D, RELU, nnz=6)
                lin(b + ".fc2", 1, 0, D, D, RELU, res=0, nnz=6)

        p.inp("kcs", 32, "bf16", ld=32)
        p.load("kcs", 1)
        lin("special_KCS_previous.0", 1, 0, D, 30, RELU)
        blocks(("special_KCS_block1", "special_KCS_block2", "special_KCS_block3"))
        m1 = p.gemm(0, 2, 100, D, NONE, nnz=4)                               # merge layer, KCS half (with the bias)
        p.inp("x", 48, "f32", ld=48)
        p.load("x", 1)
        lin("previous.0", 1, 0, D, 48, RELU)
        blocks(("block1", "block2", "block3"))
        m2 = p.gemm(0, 2, 100, D, RELU, res=2, nnz=4, b=np.zeros(100))       # pose half, added to the parked share
        p.sd["merge_previous.0.weight"], p.sd["merge_previous.0.bias"] = np.concatenate([m1["W"], m2["W"]], axis=1), m1["b"]
        lin("merge_block1.fc1", 2, 0, 100, 100, RELU)
        u = lin("merge_block1.fc2", 0, 1, 100, 100, RELU, res=2, dot="y", ld=1)
        p.sd["output.weight"], p.sd["output.bias"] = u["dotw"][None, :], np.array([u["dotb"]])
        return p
    return build


def _register_shipped():
    for D in (64, 128, 256):
        for kind, fn in (("gen", _ship_gen), ("d2", _ship_d2), ("d3", _ship_d3)):
            name = "ship_%s_D%d" % (kind, D)
            _reg("ship", name)(fn(name, D))


_register_singles()
_register_shipped()
_register_two_source()
_register_narrow()
_register_stacks()
_register_rest()
_register_real()
TIER1 = ("single", "two", "narrow", "stack", "park", "stale")


# ---- running a program on the GPU ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def environment(names_):
    old = {n: os.environ.get(n) for n in (NOPAIR, NOTAIL2, NOSTACK)}
    try:
        for n in old:
            os.environ.pop(n, None)
        for n in names_:
            os.environ[n] = "1"
        yield
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


def _to_dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda").to(dtype)


class Device:
    """the program's inputs, packed weights (through the pack entry points), biases and logit vectors on the GPU: built once"""

    def __init__(self, p, dhaug):
        import torch
        self.torch, self.p, self.lib, self.ops = torch, p, dhaug._lib, dhaug.ops
        vp = ctypes.c_void_p
        self.inputs, self.layers = {}, []
        for name, T in p.tensors.items():
            if T["data"] is None:
                continue
            dt = torch.bfloat16 if T["dtype"] == "bf16" else torch.float32
            buf = torch.full((p.mmax, T["ld"]), float("nan"), dtype=dt, device="cuda")
            buf[:, :T["width"]] = _to_dev(torch, T["data"], dt)
            self.inputs[name] = buf
        for u in p.units:
            if u["kind"] != GEMM:
                self.layers.append(None)
                continue
            N, K, K2 = u["N"], u["K"], u["K2"]
            assert u["composed"] is None                                     # (composed layers run through fused.py: test_shipped_builders_exact)
            d = {}
            bias = torch.zeros(256, dtype=torch.float32, device="cuda")
            for key, k0, k, ks in (("w", 0, K, u["ksteps"]), ("w2", K, K2, u["ksteps2"])):
                if k == 0:
                    continue
                # the blob must have the chunks the unit is handed: fewer true columns are packed from a zero-padded matrix
                kpack = k if (k + 63) // 64 == (ks + 3) // 4 else 64 * ((ks + 3) // 4)
                blob = torch.empty(8 * 4 * ((kpack + 63) // 64) * 512, dtype=torch.bfloat16, device="cuda")
                if kpack == k:                                               # a column range of the whole matrix
                    Wd = _to_dev(torch, u["W"], torch.float32)
                else:
                    Wd = torch.zeros((N, kpack), dtype=torch.float32, device="cuda")
                    Wd[:, :k] = _to_dev(torch, u["W"][:, k0:k0 + k], torch.float32)
                    k0 = 0
                self.lib.call("dhaug_pack_wfrag", vp(Wd.data_ptr()), Wd.shape[1], vp(blob.data_ptr()), N, kpack, k0, self.ops._stream())
                d[key] = blob
            bias[:N] = _to_dev(torch, u["b"], torch.float32)
            d["bias"] = bias
            if u["flags"] & F_DOT_OUT:
                v = torch.zeros(260, dtype=torch.float32, device="cuda")
                v[:N] = _to_dev(torch, u["dotw"], torch.float32)
                v[256] = u["dotb"]
                d["w2"] = v
            self.layers.append(d)
        torch.cuda.synchronize()

    def run(self, M):
        """one launch over the first M rows -> {name: the whole (M + 2, ld) NaN-filled tensor the program wrote into}"""
        torch, p = self.torch, self.p
        outs = {}
        for name, T in p.tensors.items():
            if T["data"] is None:
                dt = torch.bfloat16 if T["dtype"] == "bf16" else torch.float32
                outs[name] = torch.full((M + 2, T["ld"]), float("nan"), dtype=dt, device="cuda")
        units = []
        for u, d in zip(p.units, self.layers):
            m = self.lib.MlpUnit()
            m.kind, m.src, m.dst, m.res, m.src2 = u["kind"], u.get("src", -1), u.get("dst", -1), u.get("res", -1), u.get("src2", -1)
            if u["kind"] != GEMM:
                g = self.inputs[u["t"]] if u["t"] in self.inputs else outs[u["t"]]
                m.cols, m.ld, m.g = u["cols"], g.stride(0), g.data_ptr()
            else:
                m.flags, m.ksteps, m.ksteps2, m.n, m.act, m.slope = u["flags"], u["ksteps"], u["ksteps2"], u["N"], u["act"], u["slope"]
                m.w, m.bias = d["w"].data_ptr(), d["bias"].data_ptr()
                if "w2" in d:
                    m.w2 = d["w2"].data_ptr()
                if u["flags"]:
                    g = outs[u["t"]]
                    m.g, m.ld = g.data_ptr(), g.stride(0)
            units.append(m)
        arr = (self.lib.MlpUnit * len(units))(*units)
        with environment(p.env), self.ops.workgroup_cap(p.cap):
            self.lib.call("dhaug_mlp_forward", arr, len(units), M, self.ops._stream())
        torch.cuda.synchronize()
        return outs


def compare(p, outs, M, report=None):
    """tier 1: bit for bit; tier 2: within the reference's bound.  Everything outside the written block must still be NaN."""
    import torch
    r = p.ref()
    for name, got in outs.items():
        T = p.tensors[name]
        w = T["width"]
        g = got.float().cpu()
        assert torch.isnan(g[M:]).all(), "%s M=%d: %s has rows at or after M written" % (p.name, M, name)
        assert torch.isnan(g[:, w:]).all(), "%s M=%d: %s has columns beyond %d written" % (p.name, M, name, w)
        ref = torch.from_numpy(r["out"][name][:M])
        if p.tier == 1:
            want = ref.float()
            assert torch.equal(want.double(), ref)
            if not torch.equal(g[:M, :w], want):
                bad = (g[:M, :w] != want).nonzero()
                i, j = int(bad[0, 0]), int(bad[0, 1])
                raise AssertionError("%s M=%d: %s differs at %d places, first at row %d column %d: got %r, reference %r"
                                     % (p.name, M, name, bad.shape[0], i, j, float(g[i, j]), float(want[i, j])))
        else:
            bnd = torch.from_numpy(r["bound"][name][:M])
            err = (g[:M, :w].double() - ref).abs()
            if report is not None:
                ratio = torch.where(bnd > 0, err / bnd, err * float("inf")).nan_to_num(nan=0.0)       # (0 / 0: a padding column)
                report("%s %s: max err %.3e, max err / bound %.3f" % (p.name, name, float(err.max()), float(ratio.max())))
            assert torch.isfinite(g[:M, :w]).all()
            assert (err <= bnd).all(), "%s: %s exceeds its bound by a factor %.3f" % (p.name, name, float((err / bnd).max()))
