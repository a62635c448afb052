"""Seeded inputs, sizes and plain restatements for tests/test_gpu_stream_elem.py: the operand packing, column-sum, activation-backward,
rank-one and Adam kernels of csrc/dhaug_elem.hip.  Everything here is torch on whatever device its arguments live on and imports no
code of the package, so the references -- and the power of the comparisons built on them (tests/test_cpu_boundary.py::
test_stream_elem_references_reject_emulated_faults) -- can be checked without a GPU."""
import functools

import torch

import pose_elem_util as P

GRID_CAP, ELEMS_PER_PASS, rule, gen, maxabs = P.GRID_CAP, P.ELEMS_PER_PASS, P.rule, P.gen, P.maxabs
F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16

RAGGED_ROWS = [1, 63, 64, 65, 1000]
RAGGED_COLS = [1, 7, 8, 9, 30, 31, 33, 100, 257]


def ceil_to(v, m):
    return (v + m - 1) // m * m


# ---- one multi-pass shape per kernel: the smallest whose item count exceeds one pass of grid1d()'s GRID_CAP workgroups (dhaug_elem.hip
# :9-13), with a ragged second trip.  A changed constant in the source is a size to revisit here.
# cast_pad_kernel (dhaug_elem.hip:19-21): one lane per PAIR of the pad_cols output columns; (30 -> 32 columns: 16 pairs a row) one row
# beyond a full pass leaves 16 lanes of one workgroup for the second trip
MP_CAST_PAD = (ELEMS_PER_PASS // 16 + 1, 30, 32)                        # rows, cols, pad_cols
# cast_transpose_kernel (dhaug_elem.hip:35-36, launch :692-693): one workgroup per 32 x 32 tile of (pad_cols, cols), capped at GRID_CAP
# tiles: 2 049 x 2 = 4 098 tiles, the second trip's last tile holds 4 source rows (16 of its 32 pad columns) and 1 of 32 columns
MP_CAST_TRANSPOSE = (GRID_CAP // 2 * 32 + 4, 33, GRID_CAP // 2 * 32 + 16)   # rows, cols, pad_cols
# split_kernel (dhaug_elem.hip:65-67): one lane per 8 output columns; (9 -> 16 columns: 2 chunks a row) two rows beyond a full pass
MP_SPLIT = (ELEMS_PER_PASS // 2 + 2, 9, 16)
# act_backward_kernel (dhaug_elem.hip:196-197): one lane per 8 columns, N = 8: one chunk a row
MP_ACT_BF16 = (ELEMS_PER_PASS + 3, 8)                                   # M, N
# act_backward_f32_kernel :219, add_f32_kernel :489, adam_kernel :228, adam_dev_kernel :308: one lane per element
MP_FLAT = ELEMS_PER_PASS + 3
# rank1_mask_kernel (dhaug_elem.hip:546-548): one lane per 8 of the pad columns (N = 9 -> pad 16: 2 chunks a row)
MP_RANK1 = (ELEMS_PER_PASS // 2 + 2, 9, 16)                             # M, N, pad
# adam_nt_kernel (launch dhaug_elem.hip:780, loop :354): 4 096-element items on at most 8 192 workgroups; a 1-D parameter of
# 8 192 items + one full + one with a single element: the non-matrix branch wraps with a ragged last item
ADAM_NT_GRID, ADAM_NT_ITEM = 8192, 4096
MP_ADAM_NT = ADAM_NT_GRID * ADAM_NT_ITEM + ADAM_NT_ITEM + 1
# nn_from_nt_kernel (launch :785, loop :416-417): 64 workgroups over 64 x 64 tiles of (Np, K): a (520, 600) weight has 9 x 10 = 90
NN_TILE_WEIGHT = (520, 600)
# repack_nt_kernel / repack_nn_kernel (launch :795-796): 32 workgroups a weight; the same (520, 600) weight is 158 080 pairs (19 trips)
# and 17 x 19 = 323 tiles of 32 x 32 (11 trips)
REPACK_SHAPES = [(1, 7), NN_TILE_WEIGHT, (300, 40), (3, 1)]


def items(kernel):
    """work items of the multi-pass shape of `kernel`, and the items one pass covers (so that a test can assert the wrap)"""
    cdiv = lambda a, b: (a + b - 1) // b
    if kernel == "cast_pad":
        r, c, p = MP_CAST_PAD
        return r * p // 2, ELEMS_PER_PASS
    if kernel == "cast_transpose":
        r, c, p = MP_CAST_TRANSPOSE
        return cdiv(p, 32) * cdiv(c, 32), GRID_CAP
    if kernel == "split":
        r, c, p = MP_SPLIT
        return r * p // 8, ELEMS_PER_PASS
    if kernel == "act_bf16":
        return MP_ACT_BF16[0] * MP_ACT_BF16[1] // 8, ELEMS_PER_PASS
    if kernel == "rank1":
        return MP_RANK1[0] * MP_RANK1[2] // 8, ELEMS_PER_PASS
    if kernel == "flat":
        return MP_FLAT, ELEMS_PER_PASS
    if kernel == "adam_nt":
        return cdiv(MP_ADAM_NT, ADAM_NT_ITEM), ADAM_NT_GRID
    raise KeyError(kernel)


# --------------------------------------------------------------------------------------------------------------- comparisons
def ibits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits_nan(got, ref):
    """bit for bit, except that a NaN of the reference may be any NaN"""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    nan = torch.isnan(ref)
    return bool((torch.isnan(got) == nan).all()) and torch.equal(ibits(got)[~nan], ibits(ref)[~nan])


PAYLOAD16 = 0x7fc1                           # the NaN payload tests/test_gpu_pose_elem.py's Guarded fills 16-bit outputs with


def rows_ok(view, width, ref, nan_ok=False, payload=PAYLOAD16):
    """the comparison of a 16-bit output `view` (rows, ld) that was filled with `payload` before the launch: columns [0, width) equal
    ref bit for bit (a NaN of ref may be any NaN with nan_ok), columns [width, ld) still hold the payload"""
    got = view[:, :width]
    same = same_bits_nan(got, ref) if nan_ok else (got.shape == ref.shape and torch.equal(ibits(got), ibits(ref)))
    return bool(same) and bool((ibits(view[:, width:]) == payload).all())


def exact_sums_ok(got, x):
    """fp32 column sums `got` equal the int64 sums of the integer-valued x, whose largest magnitude stays below 2^24"""
    ref, top = colsum_exact(x)
    assert top < 2 ** 24
    return torch.equal(got.double().cpu(), ref.double().cpu())


# ------------------------------------------------------------------------------------------------------------ special values
def f32_from_bits(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(F32)


# fp32 bit patterns the casts must get right.  bf16 keeps the upper 16 bits, rounded to nearest even on the lower 16.
SPECIAL_F32 = [
    0x00000000, 0x80000000,                 # +-0
    0x7f800000, 0xff800000,                 # +-inf
    0x3f808000,                             # 1 + 2^-8: a tie, the kept part 0x3f80 is even -> rounds DOWN to 0x3f80
    0x3f818000,                             # 1 + 3 * 2^-8: a tie, the kept part 0x3f81 is odd -> rounds UP to 0x3f82
    0xbf808000, 0xbf818000,                 # the same two, negative
    0x3f808001, 0x3f807fff,                 # one ulp above / below the tie
    0x7f7f8000,                             # the smallest fp32 that rounds to bf16 +inf (a tie on the largest finite bf16, odd)
    0x7f7fffff, 0xff7fffff,                 # +-FLT_MAX -> +-inf
    0x7f7f7fff,                             # just below that tie: stays the largest finite bf16 0x7f7f
    0x00000001, 0x80000001,                 # the smallest fp32 subnormals -> +-0
    0x00008000,                             # a subnormal tie on an even kept part (0x0000) -> +0
    0x00008001,                             # just above -> the bf16 subnormal 0x0001
    0x00018000,                             # a subnormal tie on an odd kept part -> 0x0002
    0x007fffff, 0x807fffff,                 # the largest subnormals -> round up into the smallest normal 0x0080
    0x00400000, 0x00010000,                 # subnormals that bf16 holds exactly
    0x00800000,                             # the smallest normal
]
SPECIAL_F16_SAFE = [w for w in SPECIAL_F32 if (w & 0x7fffffff) < 0x477fe000]      # |x| < 65 504 (0x477fe000 = 65 504.0)
NAN_F32 = [0x7fc00000, 0xffc00000, 0x7f800001, 0x7fc0dead]                       # quiet, negative, signalling, payload


def special_matrix(rows, cols, words, seed):
    """randn (rows, cols) with the patterns of `words` planted at seeded places (every one at least once when they fit)"""
    g = gen(seed)
    x = torch.randn(rows, cols, generator=g)
    flat = x.reshape(-1)
    n = min(len(words), flat.numel())
    where = torch.randperm(flat.numel(), generator=g)[:n]
    flat[where] = f32_from_bits(words[:n])
    return x


# mask values act_backward (a float compare) and rank1_mask (a compare on the bf16 bits) must agree on: +-0, +-inf, +-the smallest
# bf16 subnormal, +-the largest finite
MASK_SPECIAL_BF16 = [0x0000, 0x8000, 0x7f80, 0xff80, 0x0001, 0x8001, 0x007f, 0x807f, 0x7f7f, 0xff7f]


def bf16_from_bits(words):
    return torch.tensor([w - (1 << 16) if w >= (1 << 15) else w for w in words], dtype=torch.int16).view(BF16)


def plant_mask(y, seed):
    """y (bf16) with every pattern of MASK_SPECIAL_BF16 planted several times at seeded places; returns y (changed in place)"""
    flat = y.reshape(-1) if y.is_contiguous() else None
    assert flat is not None
    n = flat.numel()
    reps = max(1, min(8, n // len(MASK_SPECIAL_BF16)))
    vals = bf16_from_bits(MASK_SPECIAL_BF16 * reps).to(y.device)
    where = torch.randperm(n, generator=gen(seed))[:vals.numel()].to(y.device)
    flat[where] = vals[:where.numel()]
    return y


# ------------------------------------------------------------------------------------------------------ A. packing references
def cast_pad_ref(src, pad_cols):
    """bf16 (rows, pad_cols): round to nearest even, zero beyond cols"""
    rows, cols = src.shape
    out = torch.zeros(rows, pad_cols, dtype=BF16, device=src.device)
    out[:, :cols] = src.to(BF16)
    return out


def cast_transpose_ref(src, pad_cols):
    """bf16 (cols, pad_cols) = src^T, zero beyond rows"""
    rows, cols = src.shape
    out = torch.zeros(cols, pad_cols, dtype=BF16, device=src.device)
    out[:, :rows] = src.t().to(BF16)
    return out


def split_pieces(x, half):
    """the distinct pieces of the split: bf16 hi = bf16(x), mid = bf16(x - hi), lo = bf16((x - hi) - mid); IEEE half hi, lo = f16(x - hi).
    Every residual is one fp32 subtraction."""
    dt = F16 if half else BF16
    hi = x.to(dt)
    r1 = x - hi.float()
    mid = r1.to(dt)
    if half:
        return [hi, mid]
    return [hi, mid, (r1 - mid.float()).to(dt)]


SPLIT_BF16_LAYOUT = {(0, 3): (0, 0, 1), (1, 3): (0, 1, 0), (0, 6): (0, 0, 1, 1, 0, 2), (1, 6): (0, 1, 0, 1, 2, 0), (2, 6): (0, 1, 2)}
SPLIT_F16_LAYOUT = {0: (0, 0, 1), 1: (0, 1, 0), 2: (0, 1)}


def split_ref(x, layout, pad_cols, half):
    """(rows, len(layout) * pad_cols): segment s holds piece layout[s], zero beyond cols"""
    rows, cols = x.shape
    pc = split_pieces(x, half)
    out = torch.zeros(rows, len(layout) * pad_cols, dtype=pc[0].dtype, device=x.device)
    for s, k in enumerate(layout):
        out[:, s * pad_cols:s * pad_cols + cols] = pc[k]
    return out


def act_neg(act, slope):
    return {0: 1.0, 1: 0.0, 2: slope}[act]


def act_backward_ref(g, y, act, slope):
    """g * act'(y) with a FLOAT compare y > 0, rounded to g's type (bf16 or fp32)"""
    gf = g.float()
    return torch.where(y.float() > 0, gf, gf * act_neg(act, slope)).to(g.dtype)


def rank1_ref(seed, w, y, N, pad, dneg):
    """bf16 (M, pad) = bf16(bf16(seed[r] * w[c]) * (y[r][c] > 0 ? 1 : dneg)), the weight row zero-extended to pad columns
    (seed (M,), w (N,), y (M, >= pad) bf16; finite masks only)"""
    wz = torch.zeros(pad, dtype=F32, device=w.device)
    wz[:N] = w.float()
    g = (seed.float()[:, None] * wz[None, :]).to(BF16).float()
    return torch.where(y[:, :pad].float() > 0, g, g * dneg).to(BF16)


# ----------------------------------------------------------------------------------------------------------- B. column sums
def int_matrix(M, N, seed, device="cpu"):
    """integers in [-8, 8] as fp32: exact in bf16 and fp32, every partial sum of up to 2^20 rows below 2^24"""
    return torch.randint(-8, 9, (M, N), generator=gen(seed)).float().to(device)


def colsum_exact(x):
    """the int64 column sums (as int64) and their largest magnitude"""
    s = x.to(torch.int64).sum(0)
    return s, (int(s.abs().max()) if s.numel() and x.shape[0] else 0)


def folded(x):
    """x with its second half the exact negative of the first (even row count): every column sums to exactly 0 WHEN rows r and r + M/2
    are added first, in any order of the rest"""
    M = x.shape[0]
    assert M % 2 == 0
    y = x.clone()
    y[M // 2:] = -y[:M // 2]
    return y


def colsum_emulate(x, pair):
    """fp32 column sums in the kernel's shape for an even row count: a[r] = x[r] + x[pair(r)] first, then the a's serially in fp32
    (host emulation for the fault check: pair = lambda r, h: r + h is the kernel's fold, r + 1 a wrong one)"""
    M = x.shape[0]
    h = M // 2
    s = torch.zeros(x.shape[1], dtype=F32)
    if pair(0, h) == h:
        rows = [(r, r + h) for r in range(h)]
    else:
        rows = [(r, r + 1) for r in range(0, M, 2)]
    for a, b in rows:
        s = s + (x[a] + x[b])
    return s


# ------------------------------------------------------------------------------------------------------------------- C. Adam
ADAM_LR, ADAM_BETAS, ADAM_EPS, ADAM_GSCALE = 1e-4, (0.5, 0.9), 1e-8, 0.5
ADAM_STEPS = (1, 2, 3, 1000)
ADAM_SIZES = [1, 255, 257, MP_FLAT]
T_ADAM = 2e-7                                # the bound of test_colsum_actbwd_adam


def as_f32(v):
    """the value the kernel receives for a hyperparameter passed as a C float"""
    return float(torch.tensor(v, dtype=F32))


def adam_ref(p, g, m, v, step, dtype, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, gscale=ADAM_GSCALE):
    """adam_kernel's formula (dhaug_elem.hip:224-236), expression for expression, at `dtype`: returns new (p, m, v).  The
    hyperparameters are the fp32 values the kernel receives; the bias corrections are computed in double and rounded to fp32, as
    dhaug_adam_step does, for the fp32 restatement."""
    lr, b1, b2, eps, gscale = (as_f32(x) for x in (lr, betas[0], betas[1], eps, gscale))
    bc1, bc2s = 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5
    if dtype == F32:
        bc1, bc2s = as_f32(bc1), as_f32(bc2s)
    c = lambda x: torch.tensor(x, dtype=dtype, device=p.device)
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    gi = g * c(gscale)
    mi = m + (gi - m) * (c(1.0) - c(b1))
    vi = v * c(b2) + gi * gi * (c(1.0) - c(b2))
    denom = torch.sqrt(vi) / c(bc2s) + c(eps)
    return p - (c(lr) / c(bc1)) * (mi / denom), mi, vi


ADAM_ZERO_AT = 0                             # the element with g = m = v = 0 in every step (kept where n = 1 would lose it: n > 1 only)


ADAM_GRAD_SCALES = (1.0, 0.5, 2.0, 1.5)


def adam_inputs(n, seed=5):
    """p0 (n,) randn and the gradients of the steps of ADAM_STEPS: ONE randn direction at four positive scales -- with independent
    gradients the four updates cancel at 16 % of the elements (measured on the reference: 84 % move by lr / 2), and an untouched
    element could hide among them; with a common sign every update moves its element the same way, by about lr a step.  Element
    ADAM_ZERO_AT (n > 1) has a zero gradient throughout."""
    g = gen(seed + n)
    p0 = torch.randn(n, generator=g)
    d = torch.randn(n, generator=g)
    if n > 1:
        d[ADAM_ZERO_AT] = 0.0
    return p0, [d * a for a in ADAM_GRAD_SCALES]


@functools.lru_cache(maxsize=None)
def adam_case(n):
    """inputs and the fp64 / fp32 trajectories' ends: dict(p0, grads, ref64=(p, m, v), ref32=(p, m, v)).  Computed once, shared, never
    changed by a test."""
    p0, grads = adam_inputs(n)
    out = {}
    for dt in (F64, F32):
        p, m, v = p0.to(dt), torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt)
        for step, gr in zip(ADAM_STEPS, grads):
            p, m, v = adam_ref(p, gr, m, v, step, dt)
        out[dt] = (p, m, v)
    return dict(p0=p0, grads=grads, ref64=out[F64], ref32=out[F32])


def adam_check(name, got, case, lr=ADAM_LR):
    """the three comparisons of section C on (p, m, v) `got` against `case` (adam_case or a dict of the same keys): the rule for p, m,
    v; the bound for p below lr / 10; p moved by at least lr / 2 at more than 99 % of the elements.  Returns the three bounds."""
    bounds = []
    for k, what in enumerate("pmv"):
        _, b = rule("%s %s" % (name, what), got[k], case["ref64"][k], case["ref32"][k], T_ADAM)
        bounds.append(b)
    assert bounds[0] < lr / 10.0, (name, bounds[0])
    moved = (got[0].detach().double().cpu() - case["p0"].double().cpu()).abs() >= lr / 2.0
    n = moved.numel()
    frac = moved.double().mean().item()
    print("%-58s moved by >= lr/2: %.4f of %d" % (name, frac, n))
    assert frac > 0.99, (name, frac)
    return bounds
