"""Unit-level harness of dhaug_mlp_forward_x3 (csrc/dhaug_mlp_x3.hip, mode "f16x3" of fused.py), beside tests/mlp_unit_util.py
whose helpers (lowbit, the exactness assertion, nondegenerate, the M values) it shares.  Small programs built straight from
_lib.MlpUnit, an fp64 reference of the unit semantics written from include/dhaug.h and the kernel source, and the conditions that
make a bit-for-bit comparison legitimate.  Nothing here calls the kernel under test for a value it is compared with; only Device
touches the GPU.

What the reference models, per batch row:
  * ONE image of 256 columns in two planes: a stored value v is hi = fp16(v) (round to nearest even), lo = fp16(v - hi), and every
    later use of it -- as a GEMM source or as a residual out of the register stash -- is hi + lo;
  * LOAD_F32 writes columns [0, cols) as such pairs and zeros up to the next multiple of 64; LOAD_KCS writes the 30 KCS features
    of a pose row (kcs_features, csrc/dhaug_fk_math.h: bone = child - parent joint, 15 cosines dot / (len len), 15 lengths)
    into columns 0..29 and zeros into 30..63;
  * a GEMM unit reads whole 64-column chunks [0, 64 chunks), chunks = ceil(ksteps / 4) in {1, 2, 4}, against weights that are
    zero outside N x K (dhaug_pack_wfrag_f16x2[_t16]: 8 slices, 4 chunks k-steps), and per output element adds, k ascending,
    Wlo Xhi, Whi Xlo, Whi Xhi into one fp32 accumulator seeded with the bias; Wlo Xlo is DROPPED by design, here too.  The residual
    (hi + lo from the stash) or the parked fp32 sum (workspace region 1) is added last, then the activation is applied, then the
    result is split into the image -- columns [0, 32 * 2^lg): 256 for N > 128, 128 for N > 64, 64 for N > 32, else 32, with zero
    weight rows and zero bias beyond N -- or left unrounded in the OUT_F32 tensor (the image is its staging area: undefined
    afterwards);
  * ordering: the epilogue is v = acc [+ add]; v = act(v); then the store.  A unit whose result is only ever ADDED later (never
    read as a source) parks act(v), unrounded fp32, in region 1 and leaves the image as it was (PF_TO_PARK);
  * columns a unit does not write keep what the image held.  They are "unspecified": a later unit may read them only under
    zero weights and only if they are finite (both asserted: a program that breaks this is a mistake of the test);
  * the planner (dhaug_mlp_forward_x3): where each virtual buffer's value lives -- image, stash, region 1 -- and which of the
    (chunks, map, add-mode) instantiations a unit takes.  walk() mirrors it so that a program the library would refuse fails on
    the CPU, and so that the coverage of the dispatch switch can be counted.

Tier 1 (exact), two data families:
  "int": small integer inputs, a few weights per row from {+-1/2, +-1}, integer biases, slope 2^-2: every loaded value and
         weight is an fp16 value, every lo of them is zero;
  "tp":  two-piece data: inputs a + b 2^-12 (hi = a, lo = b 2^-12), weights c + d 2^-11 with c in {+-1/2, +-1} and d in
         {0, sign(c)} where |c| = 1 (1 + 2^-11 is an fp16 tie: hi = c, lo = d 2^-11), so that the lo planes and both cross terms
         hold exactly known non-zero content.  Weights with d != 0 sit on layers fed by a LOAD (Xhi is then a small integer and
         Wlo Xhi stays within the exact window); deeper layers take weights +-1 and carry non-zero Xlo.
For every GEMM unit, row and feature the reference asserts the condition of mlp_unit_util over the three kept product terms,
the bias and the residual (sum|terms| < 2^22 q), that every stored activation equals its hi + lo and stays below 65 504, and that
every non-zero piece is a normal fp16 number (>= 2^-14).  Tier 2 is bounded instead: see test_gpu_mlp_x3_units.py."""
import ctypes

import numpy as np

import mlp_unit_util as U
from mlp_unit_util import EXACT_BITS, LRELU, M_CAP, MMAX, MS, NONE, RELU, act_fn, lowbit  # noqa: F401

LOAD_F32, GEMM, LOAD_KCS = 0, 3, 5
F_OUT_F32, F_T16 = 4, 32
OK, EINVAL, EALIGN, EUNSUPPORTED = 0, -1, -2, -3
MAP_1x4, MAP_1x2, MAP_1x1 = 1, 2, 3
PF_ADD_STASH, PF_ADD_R1, PF_KEEP, PF_TO_PARK = 1, 2, 4, 8
ADD_MODES = ("none", "keep", "r1", "stash")                               # the four instantiations per (chunks, map)
WORKSPACE_BYTES = 2 * 256 * 4 * 64 * 128 * 4                              # DHAUG_MLP_X3_WORKSPACE_BYTES
F16_MAX, F16_MIN_NORMAL = 65504.0, 2.0 ** -14
KCS_BONE_P = (5, 2, 4, 1, 0, 0, 0, 7, 8, 8, 10, 13, 11, 14, 8)
KCS_BONE_C = (6, 3, 5, 2, 4, 1, 7, 8, 10, 13, 11, 14, 12, 15, 9)
KCS_I = (0, 1, 2, 3, 4, 4, 5, 6, 7, 7, 7, 8, 9, 10, 11)
KCS_J = (2, 3, 4, 5, 5, 6, 6, 7, 14, 8, 9, 10, 11, 12, 13)


# ---- number formats ---------------------------------------------------------------------------------------------------
def f16_round(a):
    """fp64 values that are fp32 values -> nearest fp16 value, ties to even, as fp64 (|a| <= 65 504)"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


def split(v):
    hi = f16_round(v)
    return hi, f16_round(v - hi)


def is_f16(a):
    return bool(np.all(f16_round(a) == a))


def pieces_ok(what, v):
    """v (fp32 values) is carried exactly by its pair, in range, and both pieces are zero or normal -> (hi, lo)"""
    assert np.isfinite(v).all() and (np.abs(v) < F16_MAX).all(), what + ": a value leaves the fp16 range"
    hi, lo = split(v)
    assert (hi + lo == v).all(), what + ": a value does not fit the 22 bits of hi + lo"
    for q in (hi, lo):
        assert (np.abs(q[q != 0]) >= F16_MIN_NORMAL).all(), what + ": a piece is no normal fp16 number"
    return hi, lo


def pack_f16x2(W, K, k0, t16):
    """numpy form of dhaug_pack_wfrag_f16x2[_t16], from the formulas in include/dhaug.h -> fp16 bit patterns (uint16).
    W (N, ldw) fp32 values; piece 0 = fp16(w), piece 1 = fp16(w - piece 0); 0 outside N x K; ksteps = 4 ceil(K / 64); 8 slices."""
    W = np.asarray(W, dtype=np.float64)
    N = W.shape[0]
    ksteps = 4 * ((K + 63) // 64)
    P = np.zeros((256, 16 * ksteps))
    P[:N, :K] = W[:, k0:k0 + K]
    pc = np.stack(split(P))                                                 # (piece, n, k)
    if not t16:
        # dst[(((s*ksteps + ks)*2 + piece)*64 + lane)*8 + j]: n = 32 s + (lane & 31), k = 16 ks + 8 (lane >> 5) + j
        A = pc.reshape(2, 8, 32, ksteps, 2, 8).transpose(1, 3, 0, 4, 2, 5)  # (piece, s, r, ks, h, j) -> (s, ks, piece, h, r, j)
    else:
        # dst[((((s*2 + ft)*(ksteps/2) + ks)*2 + piece)*64 + lane)*8 + j]: n = 32 s + 16 ft + (lane & 15), k = 32 ks + 8 (lane >> 4) + j
        A = pc.reshape(2, 8, 2, 16, ksteps // 2, 4, 8).transpose(1, 2, 4, 0, 5, 3, 6)   # -> (s, ft, ks, piece, q, r, j)
    return np.ascontiguousarray(A).reshape(-1).astype(np.float16).view(np.uint16)


def kcs_features(pose):
    """(M, 48) -> (M, 30), the formula of kcs_features in fp64; the harness's poses make every step exact in fp32 (asserted)"""
    p = np.asarray(pose, dtype=np.float64).reshape(-1, 16, 3)
    b = p[:, list(KCS_BONE_C)] - p[:, list(KCS_BONE_P)]
    l2 = (b * b).sum(-1)
    ln = np.sqrt(l2)
    assert (ln == np.round(ln)).all() and (ln >= 1).all() and (l2 < 2 ** 20).all(), "bone lengths must be exact"
    dots = (b[:, list(KCS_I)] * b[:, list(KCS_J)]).sum(-1)
    cos = dots / (ln[:, list(KCS_I)] * ln[:, list(KCS_J)])
    assert np.isin(cos, (-1.0, 0.0, 1.0)).all(), "bones must be axis-aligned"
    return np.concatenate([cos, ln], axis=1)


def axis_poses(rng, M):
    """poses whose 15 bones are axis-aligned with integer lengths 1..8: cosines in {0, +-1}, every feature exact"""
    p = np.zeros((M, 16, 3))
    p[:, 0] = rng.integers(-8, 9, size=(M, 3))
    done = {0}
    while len(done) < 16:
        for par, c in zip(KCS_BONE_P, KCS_BONE_C):
            if par in done and c not in done:
                step = np.zeros((M, 3))
                step[np.arange(M), rng.integers(0, 3, size=M)] = rng.integers(1, 9, size=M) * rng.choice([-1.0, 1.0], size=M)
                p[:, c] = p[:, par] + step
                done.add(c)
    return p.reshape(M, 48)


# ---- programs ---------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, code, why):
        Exception.__init__(self, "%s (%d)" % (why, code))
        self.code = code


class Program:
    """a program over named global fp32 tensors; as in mlp_unit_util inputs hold mmax rows and the reference at M is the first
    M rows of the reference at mmax.  fam: "int" | "tp" (module docstring); t16: the fragment layout (DHAUG_MLP_F_T16)."""

    def __init__(self, name, seed, fam="int", t16=False, mmax=MMAX, cap=0, tier=1):
        self.name, self.rng, self.fam, self.t16, self.mmax, self.cap, self.tier = name, np.random.default_rng(seed), fam, t16, mmax, cap, tier
        self.units, self.tensors = [], {}
        self._ref, self._fresh = None, set()
        self.obs = 0                                                         # width of the image value the harness reads out

    def inp(self, name, width, ld=None, data=None, kcs=False):
        rng = self.rng
        if data is None and kcs:
            data = axis_poses(rng, self.mmax)
        elif data is None:
            a = rng.integers(-4, 5, size=(self.mmax, width)).astype(np.float64)
            if self.fam == "tp":
                a = np.where(np.abs(a) == 1, 3.0 * a, a)                     # hi = a: 0 or 2 <= |a| <= 4
                data = a + np.where(a != 0, rng.integers(-1, 2, size=a.shape) * 2.0 ** -11, 0.0)   # b in {-2, 0, 2}
            else:
                data = a
        data = np.asarray(data, dtype=np.float64).astype(np.float32).astype(np.float64)
        self.tensors[name] = dict(dtype="f32", width=width, ld=width + 2 if ld is None else ld, data=data, ncheck=0, kcs=kcs)
        return name

    def load(self, t, dst, cols=None):
        self.units.append(dict(kind=LOAD_F32, t=t, dst=dst, cols=self.tensors[t]["width"] if cols is None else cols))
        self._fresh = {dst}

    def load_kcs(self, t, dst):
        self.units.append(dict(kind=LOAD_KCS, t=t, dst=dst))
        self._fresh = set()                                                  # (features: integers, but treated as a deep source)

    def gemm(self, src, dst, N, K, act=NONE, slope=0.25, res=-1, out=None, ld=None, nnz=None, W=None, b=None, real=False,
             ksteps=None, ones=False):
        """out: name of the fp32 tensor of an OUT_F32 unit.  real (tier 2): normal weights / sqrt(K), fp32 biases.  ones: weights
        +-1 only (keeps the granularity of deep or LeakyReLU chains)."""
        rng = self.rng
        first = src in self._fresh
        if W is None and real:
            W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32).astype(np.float64)
        elif W is None:
            deep_tp = self.fam == "tp" and not first
            if nnz is None:
                nnz = 4 if deep_tp else (8 if first else 6)
            W = U.sparse_weights(rng, N, K, nnz if N >= 8 else max(nnz, 16))
            if ones or deep_tp:
                W = np.sign(W)
            elif self.fam == "tp":                                           # c + d 2^-11: d = sign(c) on half of the +-1
                W = W + np.where((np.abs(W) == 1) & (rng.random(W.shape) < 0.5), np.sign(W) * 2.0 ** -11, 0.0)
        if b is None and real:
            b = ((0.1 * rng.standard_normal(N)).astype(np.float32).astype(np.float64) + 0.1 + 2.0 ** -13).astype(np.float32).astype(np.float64)
        elif b is None:
            b = rng.integers(-1 if act == RELU else -2, 4 if act == RELU else 3, size=N).astype(np.float64)
        u = dict(kind=GEMM, src=src, dst=dst, res=res, N=N, K=K, act=act, slope=slope, W=W, b=b, flags=0,
                 ksteps=(K + 15) // 16 if ksteps is None else ksteps, real=real)
        if out is not None:
            assert out not in self.tensors
            u["flags"], u["t"] = F_OUT_F32, out
            self.tensors[out] = dict(dtype="f32", width=N, ld=N + 3 if ld is None else ld, data=None, ncheck=N)
        self.units.append(u)
        self._fresh = set()
        return u

    def observe(self, src, N):
        """read columns [0, N) of the image (the value of buffer src) out as tensor "y": one OUT_F32 unit per 64 columns whose
        weights select them (weight 1: Whi Xhi + Whi Xlo = hi + lo, exact), each in a launch of the whole program"""
        assert "y" not in self.tensors and self.obs == 0
        ch = 1 if N <= 64 else (2 if N <= 128 else 4)
        self.obs = N
        self.tensors["y"] = dict(dtype="f32", width=N, ld=N + 3, data=None, ncheck=N)
        self.units.append(dict(kind=GEMM, src=src, dst=(src + 1) % 3, res=-1, N=min(N, 64), K=64 * ch, act=NONE, slope=0.0, W=None, b=np.zeros(min(N, 64)),
                               flags=F_OUT_F32, ksteps=4 * ch, real=False, t="y", select=True))

    def ref(self):
        if self._ref is None:
            self._ref = walk(self)
        return self._ref


def _is_out(u):
    return u["kind"] == GEMM and bool(u["flags"] & F_OUT_F32)


def _uses(units, b, i):
    """how buffer b's current value is read after unit i until it is written again: 1 as a source, 2 as a residual"""
    m = 0
    for t in units[i + 1:]:
        if t["kind"] == GEMM:
            if t["src"] == b:
                m |= 1
            if t["res"] == b:
                m |= 2
            if t["dst"] == b and not _is_out(t):
                break
        elif t["dst"] == b:
            break
    return m


def shape_of(N, ksteps):
    nsl = (N + 31) // 32
    m = MAP_1x4 if nsl > 4 else (MAP_1x2 if nsl > 2 else MAP_1x1)
    lg = 3 if nsl > 4 else (2 if nsl > 2 else (1 if nsl == 2 else 0))
    return (ksteps + 3) // 4, m, lg


def walk(p):
    """the planner's walk and the fp64 evaluation in one pass over the program's mmax rows -> dict(out, bound (tier 2), bits,
    plan: per GEMM unit (chunks, map, lg, pf)).  Raises Refused where dhaug_mlp_forward_x3 returns an error."""
    M, units = p.mmax, p.units
    img, spec, imgbuf = np.full((M, 256), np.nan), np.zeros(256, dtype=bool), -1
    stash = r1 = None                                                        # dict(buf, val, shape)
    out, bound, bits, plan = {}, {}, 0.0, []
    if not any(u["kind"] == GEMM for u in units):
        raise Refused(EINVAL, "no GEMM unit")
    for i, u in enumerate(units):
        what = "%s unit %d" % (p.name, i)
        if u["kind"] in (LOAD_F32, LOAD_KCS):
            T = p.tensors[u["t"]]
            if u["kind"] == LOAD_KCS:
                assert T["width"] == 48 and T["ld"] >= 48
                data, cols = kcs_features(T["data"]), 30
            else:
                cols = u["cols"]
                assert 2 <= cols <= 256 and cols % 2 == 0 and T["ld"] % 2 == 0 and cols <= T["width"]
                data = T["data"][:, :cols]
            if imgbuf >= 0 and imgbuf != u["dst"]:
                m = _uses(units, imgbuf, i)
                if (m & 1) or ((m & 2) and not ((stash and imgbuf == stash["buf"]) or (r1 and imgbuf == r1["buf"]))):
                    raise Refused(EUNSUPPORTED, what + ": the LOAD overwrites a value that is still read from the image")
            pad = (cols + 63) & ~63
            if p.tier == 1:
                pieces_ok(what, data)
            img[:, :cols], img[:, cols:pad] = data, 0.0
            spec[:pad], spec[pad:] = True, False
            if stash and stash["buf"] == u["dst"]:
                stash = None
            if r1 and r1["buf"] == u["dst"]:
                r1 = None
            imgbuf = u["dst"]
            continue
        N, K, ks = u["N"], u["K"], u["ksteps"]
        assert 1 <= ks <= 16 and K <= 16 * ks
        if not 1 <= N <= 256:
            raise Refused(EUNSUPPORTED, what + ": N")
        if u["src"] != imgbuf:
            raise Refused(EUNSUPPORTED, what + ": the source is not what the image holds")
        chunks, mp, lg = shape_of(N, ks)
        if chunks not in (1, 2, 4):
            raise Refused(EUNSUPPORTED, what + ": three chunks")
        Wn, kp = 32 << lg, 64 * chunks
        pf, add = 0, None
        if u["res"] >= 0:
            if u["res"] == u["src"]:
                raise Refused(EINVAL, what + ": res == src")
            if stash and u["res"] == stash["buf"]:
                if stash["shape"] != (mp, lg):
                    raise Refused(EUNSUPPORTED, what + ": the stash was written under another block map")
                pf, add = PF_ADD_STASH, stash["val"]
            else:
                if not (r1 and u["res"] == r1["buf"] and r1["shape"] == (mp, lg)):
                    raise Refused(EUNSUPPORTED, what + ": the residual is in neither the stash nor region 1")
                pf, add, r1 = PF_ADD_R1, r1["val"], None
        is_out = _is_out(u)
        mdst = 0 if is_out else _uses(units, u["dst"], i)
        park = (not is_out) and bool(mdst & 2) and not (mdst & 1)
        if not park:
            m = _uses(units, u["src"], i)
            if (m & 1) or ((m & 2) and not ((stash and u["src"] == stash["buf"]) or (r1 and u["src"] == r1["buf"]))):
                raise Refused(EUNSUPPORTED, what + ": the source is read again after the image is overwritten")
        # ---- the value
        if u.get("select"):
            Nobs = p.obs
            x = img[:, :kp]
            assert np.isfinite(x).all() and spec[:Nobs].all(), what + ": observes columns that are not defined"
            out["y"], bound["y"] = x[:, :Nobs].copy(), bnd_img[:, :Nobs].copy() if p.tier == 2 else np.zeros((M, Nobs))
            y = None
        else:
            W = np.zeros((Wn, kp)); W[:N, :K] = u["W"]
            bp = np.zeros(Wn); bp[:N] = u["b"]
            x = img[:, :kp]
            assert np.isfinite(x).all(), what + ": reads columns that hold no finite value"
            assert not W[:, ~spec[:kp]].any(), what + ": nonzero weights on columns that belong to no value"
            extra = [bp] + ([add[:, :Wn]] if add is not None else [])
            if u["real"]:
                assert add is None and p.tier == 2
                pre = x @ W.T + bp
                aw, ax = np.abs(W), np.abs(x)
                S = ax @ aw.T + np.abs(bp)
                # operands carried to 2^-22 relative (2^-25 absolute where a piece is subnormal), the dropped Wlo Xlo
                # (|lo| <= 2^-11 (1 + 2^-11) of the value), and 3 K + 2 fp32 additions of a running sum below S
                eb = (3.01 * 2.0 ** -22) * (ax @ aw.T) + 1.001 * 2.0 ** -25 * (ax @ (aw != 0).T + ((ax != 0) * 1.0) @ aw.T) \
                    + 1.001 * (3 * K + 2) * 2.0 ** -24 * S
                slope = float(np.float32(u["slope"]))
                y = act_fn(pre, u["act"], slope)
                eb = eb + 2.0 ** -24 * np.abs(y)                             # (the slope's product)
            else:
                Xh, Xl = pieces_ok(what + " (source)", x)
                Wh, Wl = pieces_ok(what + " (weights)", W)
                Xe, We = np.concatenate([Xh, Xl, Xh], axis=1), np.concatenate([Wl, Wh, Wh], axis=1)
                bits = max(bits, U._exactness(what, Xe, We, extra, fmt=is_f16, fmt_name="fp16"))
                pre = Xe @ We.T
                for e in extra:
                    pre = pre + e
                assert (pre.astype(np.float32).astype(np.float64) == pre).all()
                y = act_fn(pre, u["act"], u["slope"])
                assert (y.astype(np.float32).astype(np.float64) == y).all(), what + ": the activation is no fp32 value"
                eb = np.zeros_like(y)
        # ---- where it goes
        if is_out:
            if not (N <= 64 and p.tensors[u["t"]]["ld"] >= N):
                raise Refused(EUNSUPPORTED, what + ": OUT_F32 shape")
            if pf:
                raise Refused(EUNSUPPORTED, what + ": OUT_F32 adds a residual")
            if y is not None:
                out[u["t"]], bound[u["t"]] = y[:, :N].copy(), eb[:, :N].copy()
            img[:], spec[:], imgbuf = np.nan, False, -1
        else:
            if u["dst"] == u["src"]:
                raise Refused(EINVAL, what + ": dst == src")
            if park:
                if r1:
                    raise Refused(EUNSUPPORTED, what + ": a second value parked while one waits")
                pf |= PF_TO_PARK
                r1 = dict(buf=u["dst"], val=y.copy(), shape=(mp, lg))
                if stash and stash["buf"] == u["dst"]:
                    stash = None
            else:
                if p.tier == 1:
                    pieces_ok(what + " (result)", y)
                else:
                    bnd_img = np.zeros((M, 256))
                    bnd_img[:, :Wn] = eb + 2.0 ** -22 * np.abs(y) + 2.0 ** -25       # the split of the stored value
                img[:, :Wn] = y
                spec[:Wn], spec[Wn:] = True, False
                if mdst & 2:
                    if stash and stash["buf"] != u["dst"] and (_uses(units, stash["buf"], i) & 2):
                        raise Refused(EUNSUPPORTED, what + ": the stash still holds a value that is added later")
                    pf |= PF_KEEP
                    stash = dict(buf=u["dst"], val=y.copy(), shape=(mp, lg))
                else:
                    if stash and stash["buf"] == u["dst"]:
                        stash = None
                    if pf & (PF_ADD_STASH | PF_ADD_R1):
                        # the adding instantiations always keep: whatever the stash held is overwritten
                        if stash and (_uses(units, stash["buf"], i) & 2):
                            raise Refused(EUNSUPPORTED, what + ": an adding layer overwrites a stash value that is added later")
                        stash = None
                if r1 and r1["buf"] == u["dst"]:
                    r1 = None
                imgbuf = u["dst"]
        plan.append(dict(unit=i, chunks=chunks, map=mp, lg=lg, pf=pf,
                         add=("r1" if pf & PF_ADD_R1 else "stash" if pf & PF_ADD_STASH else "keep" if pf & PF_KEEP else "none")))
    return dict(out=out, bound=bound, bits=bits, plan=plan)


# ---- the program families ---------------------------------------------------------------------------------------------
REG = {}
_CACHE = {}
_RETRY = ("constant over", "are equal", "must keep it below", "22 bits", "normal fp16", "fp16 range")


def _reg(family, name, fn):
    assert name not in REG
    REG[name] = (family, fn)


def get(name):
    """as mlp_unit_util.get: the data are drawn again from the next seed until the exactness conditions hold and the outputs are
    not degenerate; what comes back is asserted once more, in full, by tests/test_mlp_x3_units_cpu.py"""
    if name not in _CACHE:
        for attempt in range(16):
            p = REG[name][1](attempt)
            try:
                p.ref()
                nondegenerate(p)
                break
            except AssertionError as e:
                if attempt == 15 or not any(m in str(e) for m in _RETRY):
                    raise
        _CACHE[name] = p
    return _CACHE[name]


def nondegenerate(p):
    """mlp_unit_util.nondegenerate; a program marked few_inputs (K = 2: twenty distinct columns at most) may repeat a column"""
    try:
        U.nondegenerate(p)
    except AssertionError as e:
        if not (getattr(p, "few_inputs", False) and "are equal" in str(e)):
            raise


def names(family):
    return [n for n, (f, _) in REG.items() if f == family]


def _variants(family, base, build, fams=("int", "tp"), layouts=(False, True), **kw):
    """register build(p, ...) in both data families and both fragment layouts"""
    for fam in fams:
        for t16 in layouts:
            name = "%s_%s_%s" % (base, fam, "t16" if t16 else "t32")

            def make(attempt=0, name=name, fam=fam, t16=t16):
                p = Program(name, U._seed(name) + attempt, fam=fam, t16=t16, **kw)
                build(p)
                return p
            _reg(family, name, make)


_ACTS = (NONE, RELU, LRELU)
K1 = (2, 30, 48, 64, 66, 128, 200, 256)
N1 = (1, 33, 35, 64, 65, 100, 128, 129, 225, 256)


def _single(K, N, act, out_f32, ld_extra):
    def build(p):
        p.few_inputs = K < 30
        p.inp("x", K, ld=K + ld_extra)
        p.load("x", 1)
        if out_f32:
            p.gemm(1, 0, N, K, act, out="y", ld=N + 3)
        else:
            p.gemm(1, 0, N, K, act)
            p.observe(0, N)
    return build


def _register_singles():
    i = 0
    for iK, K in enumerate(K1):
        for iN, N in enumerate(N1):
            act = _ACTS[(iK + iN) % 3]
            _variants("single", "single_K%d_N%d_a%d" % (K, N, act), _single(K, N, act, N <= 64 and (iK + iN) % 2 == 0, 0 if i % 3 == 0 else 6))
            i += 1
    for N, K, act in ((1, 64, LRELU), (33, 128, NONE), (35, 256, RELU), (64, 30, LRELU), (64, 200, NONE)):   # every N <= 64 both ways
        _variants("single", "single_x_K%d_N%d_a%d" % (K, N, act), _single(K, N, act, True, 4))
    _variants("cap", "single_cap", _single(200, 225, LRELU, False, 6), mmax=M_CAP, cap=2)


_MID = {1: 48, 2: 100, 4: 200}                                              # a width whose consumer reads that many chunks
_KOF = {1: 30, 2: 66, 4: 200}
_NOF = {MAP_1x4: 225, MAP_1x2: 100, MAP_1x1: 35}


def _residual(ck, mp, cadd, twice=False):
    """keeper (ck chunks, map mp, result kept) -> one or two layers that overwrite the image -> the layer that adds the keeper
    (cadd chunks, map mp) -> read out"""
    def build(p):
        N, K = _NOF[mp], _KOF[ck]
        p.inp("x", K)
        p.load("x", 1)
        p.gemm(1, 0, N, K, RELU)
        if twice:
            p.gemm(0, 1, 64, N, NONE, ones=True)
            p.gemm(1, 2, _MID[cadd], 64, RELU, ones=True)
            p.gemm(2, 1, N, _MID[cadd], NONE, res=0, ones=True)
            p.observe(1, N)
        else:
            p.gemm(0, 1, _MID[cadd], N, RELU, ones=True)
            p.gemm(1, 2, N, _MID[cadd], NONE, res=0, ones=True)
            p.observe(2, N)
    return build


def _res_chain(N, K):
    """the critics' shape: a lead layer and two residual blocks (fc1, fc2 + the block's input, in place)"""
    def build(p):
        p.inp("x", K)
        p.load("x", 1)
        p.gemm(1, 0, N, K, RELU)
        for _ in range(2):
            p.gemm(0, 1, N, N, RELU, ones=True, nnz=4)
            p.gemm(1, 0, N, N, RELU, res=0, ones=True, nnz=4)
        p.observe(0, N)
    return build


def _fresh_adder(mp, ck):
    """the adding layer fed by a LOAD: its weights carry non-zero lo pieces in the two-piece family"""
    def build(p):
        N, K = _NOF[mp], _KOF[ck]
        p.inp("x", 48)
        p.load("x", 1)
        p.gemm(1, 0, N, 48, RELU)                                            # kept: read by the next layer and added by the last
        p.gemm(0, 2, 64, N, NONE, ones=True)
        p.inp("z", K)
        p.load("z", 1)
        p.gemm(1, 2, N, K, LRELU, res=0)
        p.observe(2, N)
    return build


def _register_residuals():
    for mp in (MAP_1x4, MAP_1x2, MAP_1x1):
        for j, ck in enumerate((1, 2, 4)):
            cadd = (1, 2, 4)[(j + mp) % 3]
            _variants("res", "res_m%d_k%d_a%d" % (mp, ck, cadd), _residual(ck, mp, cadd))
        _variants("res", "res_twice_m%d" % mp, _residual(2, mp, (4, 1, 2)[mp - 1], twice=True))
        _variants("res", "res_fresh_m%d" % mp, _fresh_adder(mp, (2, 4, 1)[mp - 1]))
    for N, K in ((256, 48), (100, 30), (64, 66)):
        _variants("res", "res_chain_N%d" % N, _res_chain(N, K))
    _variants("cap", "res_cap", _residual(2, MAP_1x4, 4), mmax=M_CAP, cap=2)


def _park(mp, cpark, cadd):
    """the 3D critic's merge: branch A's share of a layer is parked (fp32, region 1) while branch B runs, then added"""
    def build(p):
        N = _NOF[mp]
        p.inp("a", 30)
        p.load("a", 1)
        p.gemm(1, 0, _MID[cpark], 30, RELU)
        p.gemm(0, 2, N, _MID[cpark], NONE, ones=True)                        # parked: act(v) unrounded, the image stays
        p.inp("b", 48)
        p.load("b", 1)
        p.gemm(1, 0, _MID[cadd], 48, RELU)
        p.gemm(0, 2, N, _MID[cadd], RELU, res=2, ones=True, b=np.zeros(N))   # + the parked sum
        p.observe(2, N)
    return build


def _register_parks():
    for mp in (MAP_1x4, MAP_1x2, MAP_1x1):
        for j, cadd in enumerate((1, 2, 4)):
            _variants("park", "park_m%d_p%d_a%d" % (mp, (1, 2, 4)[(j + mp + 1) % 3], cadd), _park(mp, (1, 2, 4)[(j + mp + 1) % 3], cadd))
    _variants("cap", "park_cap", _park(MAP_1x2, 4, 4), mmax=M_CAP, cap=2)


def _kcs(N):
    def build(p):
        p.inp("pose", 48, ld=50, kcs=True)
        p.load_kcs("pose", 1)
        p.gemm(1, 0, N, 30, RELU)
        p.gemm(0, 1, 100, N, LRELU, ones=True)
        p.observe(1, 100)
    return build


def _stale(p):
    p.inp("x", 64)
    p.load("x", 1)
    big = (p.rng.integers(16, 64, size=256) * 4.0) * p.rng.choice([-1.0, 1.0], size=256)
    big[:64] = p.rng.integers(-2, 3, size=64)
    p.gemm(1, 0, 256, 64, NONE, b=big)                                       # large finite values in columns 64..255
    p.gemm(0, 1, 33, 64, RELU, ones=True)                                    # columns [0, 64) rewritten, the rest stale
    p.gemm(1, 0, 64, 33, LRELU, ones=True)                                   # reads ONE chunk: zero weights on 33..63
    p.observe(0, 64)


def _register_rest():
    for N in (256, 64):
        _variants("kcs", "kcs_N%d" % N, _kcs(N), fams=("int",))
    _variants("cap", "kcs_cap", _kcs(128), fams=("int",), mmax=M_CAP, cap=2)
    _variants("stale", "stale_columns", _stale)
    _variants("cap", "stale_cap", _stale, mmax=M_CAP, cap=2)


# the shipped builders' f16x3 programs (fused.py: GEN on the 32 x 32 body, D2 and D3 on the 16 x 16 body) unit by unit, with
# the parameters kept as a state_dict (p.sd)
def _lin(p, key, *a, **kw):
    u = p.gemm(*a, **kw)
    p.sd[key + ".weight"], p.sd[key + ".bias"] = u["W"], u["b"]
    return u


def _ship_gen(D):
    def build(p):
        p.sd = {}
        p.inp("z", 128, ld=128)
        p.load("z", 1)
        _lin(p, "preprocess.0", 1, 0, D, 128, RELU)
        for b in ("block1", "block2", "block3"):
            _lin(p, b + ".fc1", 0, 1, D, D, RELU, nnz=4, ones=True)
            _lin(p, b + ".fc2", 1, 0, D, D, RELU, res=0, nnz=4, ones=True)
        _lin(p, "deconv_out", 0, 1, 35, D, NONE, out="y", ld=35, nnz=4, ones=True)
    return build


def _ship_d2(D):
    def build(p):
        p.sd = {}
        p.inp("x", 32, ld=32)
        p.load("x", 1)
        _lin(p, "pose_layer_1", 1, 0, D, 32, LRELU, ones=True)
        _lin(p, "pose_layer_2", 0, 1, D, D, LRELU, nnz=4, ones=True)
        _lin(p, "pose_layer_3", 1, 0, D, D, LRELU, res=0, nnz=4, ones=True)
        _lin(p, "pose_layer_4", 0, 1, D, D, NONE, nnz=4, ones=True)
        _lin(p, "layer_last", 1, 0, D, D, LRELU, nnz=4, ones=True)
        _lin(p, "layer_pred", 0, 1, 1, D, NONE, out="y", ld=1, nnz=16, ones=True)
    return build


def _ship_d3(D):
    def build(p):
        p.sd = {}
        dn = 2 if p.fam == "tp" else 4                                     # (nineteen layers deep: the two-piece family keeps S small)

        def blocks(ns):
            for b in ns:
                _lin(p, b + ".fc1", 0, 1, D, D, RELU, nnz=dn, ones=True)
                _lin(p, b + ".fc2", 1, 0, D, D, RELU, res=0, nnz=dn, ones=True)

        p.inp("kcs", 30, ld=30)                                              # the fp32 (N, 30) features
        p.load("kcs", 1)
        _lin(p, "special_KCS_previous.0", 1, 0, D, 30, RELU)
        blocks(("special_KCS_block1", "special_KCS_block2", "special_KCS_block3"))
        m1 = p.gemm(0, 2, 100, D, NONE, nnz=dn, ones=True)                    # merge layer, KCS half (with the bias): parked
        p.inp("x", 48, ld=48)
        p.load("x", 1)
        _lin(p, "previous.0", 1, 0, D, 48, RELU)
        blocks(("block1", "block2", "block3"))
        m2 = p.gemm(0, 2, 100, D, RELU, res=2, nnz=dn, ones=True, b=np.zeros(100))
        p.sd["merge_previous.0.weight"], p.sd["merge_previous.0.bias"] = np.concatenate([m1["W"], m2["W"]], axis=1), m1["b"]
        _lin(p, "merge_block1.fc1", 2, 0, 100, 100, RELU, nnz=dn, ones=True)
        _lin(p, "merge_block1.fc2", 0, 1, 100, 100, RELU, res=2, nnz=dn, ones=True)
        _lin(p, "output", 1, 0, 1, 100, NONE, out="y", ld=1, nnz=16, ones=True)
    return build


def _register_shipped():
    for D in (64, 128, 256):
        _variants("ship", "ship_gen_D%d" % D, _ship_gen(D), layouts=(False,))
        # (the 2D critic has four LeakyReLU levels: 2^-8 of granularity, which the two-piece inputs' 2^-11 cannot afford with
        # every lo piece normal -- integer family only)
        _variants("ship", "ship_d2_D%d" % D, _ship_d2(D), fams=("int",), layouts=(True,))
        _variants("ship", "ship_d3_D%d" % D, _ship_d3(D), layouts=(True,))


# tier 2: one unit per (layout, chunks, map) with realistic values, M = 129
def _real(K, N):
    def build(p):
        p.inp("x", K, data=p.rng.standard_normal((p.mmax, K)))
        p.load("x", 1)
        if N <= 64:
            p.gemm(1, 0, N, K, LRELU, slope=0.01, real=True, out="y")
        else:
            p.gemm(1, 0, N, K, LRELU, slope=0.01, real=True)
            p.observe(0, N)
    return build


def _register_real():
    for K in (50, 100, 256):
        for N in (35, 100, 225):
            _variants("real", "real_K%d_N%d" % (K, N), _real(K, N), fams=("int",), mmax=129, tier=2)


_register_singles()
_register_residuals()
_register_parks()
_register_rest()
_register_shipped()
_register_real()
TIER1 = ("single", "res", "park", "kcs", "stale")


def coverage(t16):
    """{(chunks, map, add-mode)} that the registered programs of one fragment layout reach"""
    seen = set()
    for n in REG:
        p = get(n)
        if p.t16 == t16:
            seen |= {(g["chunks"], g["map"], g["add"]) for g in p.ref()["plan"]}
    return seen


# ---- running a program on the GPU ---------------------------------------------------------------------------------------
def _dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


class Device:
    """the program's inputs, packed weights (through the pack entry points) and biases on the GPU: built once.  ws: the 64 MB
    workspace, allocated once per test module."""

    def __init__(self, p, dhaug, ws):
        import torch
        self.torch, self.p, self.lib, self.ops, self.ws = torch, p, dhaug._lib, dhaug.ops, ws
        assert ws.numel() * ws.element_size() >= WORKSPACE_BYTES
        self.inputs, self.layers = {}, []
        for name, T in p.tensors.items():
            if T["data"] is not None:
                buf = torch.full((p.mmax, T["ld"]), float("nan"), dtype=torch.float32, device="cuda")
                buf[:, :T["width"]] = _dev32(torch, T["data"])
                self.inputs[name] = buf
        for u in p.units:
            if u["kind"] != GEMM:
                self.layers.append(None)
                continue
            d = dict(bias=torch.zeros(256, dtype=torch.float32, device="cuda"))
            d["bias"][:u["N"]] = _dev32(torch, u["b"])
            if u.get("select"):                                              # one blob per group of 64 observed columns
                d["w"] = []
                for g in range((p.obs + 63) // 64):
                    n = min(64, p.obs - 64 * g)
                    W = np.zeros((n, u["K"]))
                    W[np.arange(n), 64 * g + np.arange(n)] = 1.0
                    d["w"].append((n, self.pack(W, u["K"])))
            else:
                d["w"] = self.pack(u["W"], u["K"])
            self.layers.append(d)
        torch.cuda.synchronize()

    def pack(self, W, K):
        torch = self.torch
        Wd = _dev32(torch, W)
        blob = torch.empty(2 * 8 * 4 * ((K + 63) // 64) * 512, dtype=torch.float16, device="cuda")
        self.lib.call("dhaug_pack_wfrag_f16x2_t16" if self.p.t16 else "dhaug_pack_wfrag_f16x2", ctypes.c_void_p(Wd.data_ptr()), Wd.shape[1],
                      ctypes.c_void_p(blob.data_ptr()), W.shape[0], K, 0, self.ops._stream())
        return blob

    def run(self, M, features=None):
        """launches over the first M rows -> {name: the whole (M + 2, ld) NaN-filled tensor the program wrote into}; a program
        that is read out takes one launch per 64 observed columns.  features: an fp32 (M, >= 30) tensor that replaces the poses
        of every LOAD_KCS unit through a LOAD_F32 of 30 columns."""
        torch, p = self.torch, self.p
        outs = {n: torch.full((M + 2, T["ld"]), float("nan"), dtype=torch.float32, device="cuda")
                for n, T in p.tensors.items() if T["data"] is None}
        t16 = F_T16 if p.t16 else 0
        for g in range(max(1, (p.obs + 63) // 64)):
            units, keep = [], []
            for u, d in zip(p.units, self.layers):
                m = self.lib.MlpUnit()
                m.kind, m.src, m.dst, m.res, m.src2 = u["kind"], u.get("src", -1), u.get("dst", -1), u.get("res", -1), -1
                if u["kind"] == LOAD_KCS and features is not None:
                    m.kind, m.cols, m.ld, m.g = LOAD_F32, 30, features.stride(0), features.data_ptr()
                elif u["kind"] != GEMM:
                    t = self.inputs[u["t"]]
                    m.cols, m.ld, m.g = u.get("cols", 0), t.stride(0), t.data_ptr()
                else:
                    m.flags, m.ksteps, m.n, m.act, m.slope = u["flags"] | t16, u["ksteps"], u["N"], u["act"], u["slope"]
                    m.bias, m.g = d["bias"].data_ptr(), self.ws.data_ptr()
                    if u.get("select"):
                        n, blob = d["w"][g]
                        view = outs["y"][:, 64 * g:]
                        m.n, m.w, m.g, m.ld = n, blob.data_ptr(), view.data_ptr(), outs["y"].stride(0)
                        keep.append(view)
                    else:
                        m.w = d["w"].data_ptr()
                        if u["flags"] & F_OUT_F32:
                            m.g, m.ld = outs[u["t"]].data_ptr(), outs[u["t"]].stride(0)
                units.append(m)
            arr = (self.lib.MlpUnit * len(units))(*units)
            with self.ops.workgroup_cap(p.cap):
                self.lib.call("dhaug_mlp_forward_x3", arr, len(units), M, self.ops._stream())
        torch.cuda.synchronize()
        return outs


def compare(p, outs, M, report=None):
    """tier 1: bit for bit; tier 2: within the reference's bound.  Everything outside the written block must still be NaN."""
    U.compare(p, outs, M, report=report)
