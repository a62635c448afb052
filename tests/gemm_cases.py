"""The shapes at which every NT / TN GEMM route of csrc/dhaug_gemm.hip and csrc/dhaug_gemm_p8.hip is run (tests/test_gpu_gemm_routes.py)
and at which the routes themselves are pinned on the host (tests/test_cpu_boundary.py::test_gemm_case_table_reaches_every_route).

A record says what is launched (shape, row strides, which operands and outputs exist, the dispatcher's test switches) and which kernel
that launch is MEANT to reach, spelled as in csrc/dhaug_gemm_route.h (enum NtKernel / TnKernel, KSTEPS = K / 16 for the two templated
kernels).  Each case is the smallest shape that still crosses the edge in question: one row, one row short of / beyond a tile, a ragged
last column piece, every K / 16 a kernel is instantiated for, every pipeline prologue, a K tail.  Nothing here imports torch.

Strides (elements).  Every operand is a column block of a wider buffer, so a row stride is the width + 16 or more: bf16 strides are
multiples of 8 and fp32 strides multiples of 4 (16-byte aligned rows), except where a case asks for an odd fp32 output stride."""
from dataclasses import dataclass
from typing import Optional, Tuple

NT_KERNELS = ["NT256S", "WS", "P8", "WIDE", "BIG", "PIPE2", "GENERIC_128x128", "GENERIC_128x64", "GENERIC_128x32"]   # enum NtKernel
TN_KERNELS = ["TN64", "TN_GENERIC"]                                                                                 # enum TnKernel
WS_KSTEPS = (1, 2, 3, 4, 7, 8, 16)
NT256S_KSTEPS = (8, 16)
SWITCHES = ("DHAUG_GEMM_WIDE_MIN_TILES", "DHAUG_GEMM_NOP8", "DHAUG_GEMM_NO256", "DHAUG_GEMM_NOBIG")


def ceil_to(v, m):
    return (v + m - 1) // m * m


@dataclass(frozen=True)
class NtCase:
    M: int
    N: int
    K: int
    kernel: str                          # the NtKernel this launch is meant to reach
    ksteps: int                          # its KSTEPS (NT256S, WS), else 0
    bias: bool = False
    bias_off: int = 0                    # bytes the bias pointer is moved off its 16-byte alignment
    res: Optional[str] = None            # residual: None / "bf16" / "f32"
    mask: Optional[str] = None           # activation-backward mask: None / "bf16" (gemm_nt_dmask) / "f32" (gemm_nt_dmask_f32)
    act: int = 0                         # the layer's activation -- of the mask's layer where a mask is present (then 1 or 2)
    slope: float = 0.0
    out_bf16: bool = False
    out_f32: bool = False
    n_pad: int = 0                       # bf16 output: columns [N, n_pad) are written as zeros (0: none)
    lda: int = 0
    ldb: int = 0
    ld_res: int = 0
    ld_mask: int = 0
    ldc_bf16: int = 0
    ldc_f32: int = 0
    env: Tuple[Tuple[str, str], ...] = ()
    p8_ok: Optional[bool] = None         # dhaug_p8_supported() of this launch; None: the route of this case does not read it
    why: str = ""

    @property
    def W(self):                         # output width covered by tiles, as the dispatcher computes it
        return max(self.N, self.n_pad) if self.out_bf16 else self.N

    @property
    def bf16_width(self):
        return max(self.N, self.n_pad)

    @property
    def ident(self):
        tags = []
        if self.bias:
            tags.append("bias+%d" % self.bias_off if self.bias_off else "bias")
        if self.res:
            tags.append("res" + self.res)
        if self.mask:
            tags.append("mask" + self.mask)
        tags.append("act%d" % self.act)
        tags.append(("b" if self.out_bf16 else "") + ("f" if self.out_f32 else ""))
        if self.n_pad:
            tags.append("pad%d" % self.n_pad)
        if self.ldc_f32 & 3:
            tags.append("ldcf%d" % self.ldc_f32)
        tags += ["%s=%s" % (k.replace("DHAUG_GEMM_", ""), v) for k, v in self.env]
        return "%s%s-%dx%dx%d-%s" % (self.kernel, self.ksteps or "", self.M, self.N, self.K, "-".join(tags))

    def route_args(self, p8_ok):
        """the arguments of tests/hostcheck's hostcheck_nt_route for this launch"""
        env = dict(self.env)
        return (self.M, self.N, self.W, self.K, int(self.out_bf16), int(self.out_f32), int(self.res == "f32"),
                int(not (self.bias and self.bias_off % 16)), int(self.mask == "f32"), int(p8_ok),
                int("DHAUG_GEMM_NO256" in env), int("DHAUG_GEMM_NOBIG" in env), int("DHAUG_GEMM_NOP8" in env),
                int(env.get("DHAUG_GEMM_WIDE_MIN_TILES", -1)))


def odd4(N):
    """an fp32 row stride that is no multiple of 4: the element-wise store path, (ldc_f32 & 3) != 0"""
    return ceil_to(N, 4) + 17


def nt(kernel, ksteps, M, N, K, form="plain", act=0, n_pad=0, ldc_f32=0, env=(), p8_ok=None, bias_off=0, bias=None, f32=True, why=""):
    """One record.  form: plain | biasact (bias + activation) | full (bias + bf16 residual + activation) -- these three with a bf16
    output where n_pad is given, and with the fp32 output from the same launch unless f32=False (every case whose route allows it
    asks for the fp32 output: a bf16-only check cannot see one dropped k-term) | resf (bias + fp32 residual, fp32 out) |
    maskb / maskb_res (bf16 mask: bf16 out, zero-padded to n_pad) | maskf / maskf_res (fp32 mask, fp32 out).  bias: override."""
    kw = dict(bias=False, res=None, mask=None, out_bf16=False, out_f32=True)
    if form in ("plain", "biasact", "full"):
        assert n_pad or f32
        kw.update(bias=form != "plain", res="bf16" if form == "full" else None, out_bf16=bool(n_pad), out_f32=f32)
    elif form == "resf":
        kw.update(bias=True, res="f32")
    elif form in ("maskb", "maskb_res"):
        assert act in (1, 2) and 0 < n_pad <= ceil_to(N, 16), "gemm_nt_dmask pads to at most ceil16(N)"
        kw.update(mask="bf16", res="bf16" if form.endswith("res") else None, out_bf16=True, out_f32=False)
    elif form in ("maskf", "maskf_res"):
        assert act in (1, 2)
        kw.update(mask="f32", res="f32" if form.endswith("res") else None)
    else:
        raise ValueError(form)
    if bias is not None:
        kw["bias"] = bias
    if not kw["out_bf16"]:
        n_pad = 0                        # (a pad width given for a form without a bf16 output means nothing)
    assert n_pad == 0 or n_pad >= N
    width = max(N, n_pad)
    ld = {"bf16": ceil_to(N, 8) + 16, "f32": ceil_to(N, 4) + 16, None: 0}
    assert set(k for k, _ in env) <= set(SWITCHES)
    return NtCase(M=M, N=N, K=K, kernel=kernel, ksteps=ksteps, bias_off=bias_off, act=act, slope=0.01 if act == 2 else 0.0, n_pad=n_pad,
                  lda=K + 24, ldb=K + 16, ld_res=ld[kw["res"]], ld_mask=ld[kw["mask"]],
                  ldc_bf16=ceil_to(width, 8) + 16 if kw["out_bf16"] else 0, ldc_f32=(ldc_f32 or ceil_to(N, 4) + 16) if kw["out_f32"] else 0,
                  env=tuple(env), p8_ok=p8_ok, why=why, **kw)


NT_CASES = []

# ---- NT256S: gemm_nt256s_kernel<K / 16, MODE>, N = 256, bf16 in and bf16 out, whole 64-row tiles.  One and three 64-row tiles (two
# and six of the kernel's 32-row tiles: the ring of operand images is 3 or 4 deep), each of launch_nt256s' four modes: plain (0),
# + bf16 residual (1), bf16 mask (2), mask + residual (3); the first two with and without bias and with each activation.
for ks in NT256S_KSTEPS:
    for M in (64, 192):
        for form in ("plain", "full"):
            for bias in (False, True):
                for act in (0, 1, 2):
                    NT_CASES.append(nt("NT256S", ks, M, 256, 16 * ks, form, act=act, n_pad=256, bias=bias, f32=False))
        NT_CASES.append(nt("NT256S", ks, M, 256, 16 * ks, "maskb", act=1, n_pad=256))
        NT_CASES.append(nt("NT256S", ks, M, 256, 16 * ks, "maskb_res", act=2, n_pad=256))

# ---- WS: gemm_nt_ws_kernel<K / 16> (64 x 128 tiles, the weight rows resident in registers), every instantiation.  One row, one row
# short of / beyond a row tile, several row tiles; a ragged second column tile (N = 65: one column of it), a ragged column piece
# (N = 100: columns 96 .. 99 of a piece), whole tiles (N = 256).
for i, ks in enumerate(WS_KSTEPS):
    for j, M in enumerate((1, 63, 65, 300)):
        NT_CASES.append(nt("WS", ks, M, 65, 16 * ks, "plain", ldc_f32=odd4(65), why="odd fp32 row stride"))
        NT_CASES.append(nt("WS", ks, M, 100, 16 * ks, "plain", n_pad=(112, 128)[(i + j) % 2]))
        NT_CASES.append(nt("WS", ks, M, 256, 16 * ks, "plain", n_pad=256))
for i, ks in enumerate((1, 4, 7, 16)):
    for j, (M, N, n_pad) in enumerate(((65, 100, 112), (300, 256, 256), (63, 65, 80), (1, 100, 128))):
        NT_CASES.append(nt("WS", ks, M, N, 16 * ks, "full", act=1 + (i + j) % 2, n_pad=n_pad))
for ks in (4, 16):
    for M, N in ((65, 100), (300, 65), (63, 256)):
        NT_CASES.append(nt("WS", ks, M, N, 16 * ks, "resf", act=1, ldc_f32=odd4(65) if N == 65 else 0))
for i, ks in enumerate((2, 8, 16)):
    for j, (M, N, n_pad) in enumerate(((65, 100, 112), (300, 256, 256), (63, 65, 80))):
        NT_CASES.append(nt("WS", ks, M, N, 16 * ks, ("maskb", "maskb_res")[(i + j) % 2], act=1 + (i + j + 1) % 2, n_pad=n_pad))
# the 256-wide training layer with its own kernel switched off (whole 64-row tiles: NT256S otherwise)
NT_CASES.append(nt("WS", 16, 192, 256, 256, "maskb_res", act=1, n_pad=256, env=(("DHAUG_GEMM_NO256", "1"),)))
NT_CASES.append(nt("WS", 8, 64, 256, 128, "full", act=2, n_pad=256, env=(("DHAUG_GEMM_NO256", "1"),)))
# The persistent loop.  launch_ws starts gx = 2 * 256 / ntiles workgroups per column tile (two per CU over the whole grid), capped at
# the number of row tiles.  N = 1000 is ntiles = 8 column tiles of 128, so gx = 64; M = 4161 is 66 row tiles of 64.  66 > 64: workgroups
# 0 and 1 of every column tile wrap (mt += gridDim.x) to row tiles 64 and 65, and tile 65 holds ONE row (4161 = 65 * 64 + 1); the
# eighth column tile is ragged too (1000 = 7 * 128 + 104).  (4173, 512, 256) of test_gemm_nt_plain is 66 row tiles against 128 workgroups.
NT_CASES.append(nt("WS", 16, 4161, 1000, 256, "plain", n_pad=1008, why="persistent loop wraps onto a one-row tile"))
NT_CASES.append(nt("WS", 16, 4161, 1000, 256, "full", act=2, n_pad=1008, why="persistent loop wraps onto a one-row tile"))

# ---- PIPE2: gemm_nt_pipe2_kernel (64 x 64 tiles, four 64-wide K-stages buffered or in flight).  K = 80, 96: 2 stages (tails of 16 and
# 32 columns), 144: 3 stages (16), 208: 4 (16), 272: 5 (16), 1008: 16 (48) -- the three vmcnt prologues (2, 3, >= 4 stages), the first
# stage count at which a buffer is refilled (5), and a short last stage that re-reads the last full window every time.
PIPE2_K = (80, 96, 144, 208, 272, 1008)
PIPE2_EPI = ((65, 100, 112), (200, 315, 320), (63, 65, 80), (1, 315, 320))
for i, K in enumerate(PIPE2_K):
    for j, M in enumerate((1, 63, 65, 200)):
        NT_CASES.append(nt("PIPE2", 0, M, 65, K, "plain", ldc_f32=odd4(65)))
        NT_CASES.append(nt("PIPE2", 0, M, 100, K, "plain", n_pad=(112, 128)[(i + j) % 2]))
        NT_CASES.append(nt("PIPE2", 0, M, 315, K, "plain", ldc_f32=odd4(315) if j % 2 else 0))
    for j, form in enumerate(("full", "resf", "maskb", "maskb_res")):          # every form at every stage count, the shapes in turn
        M, N, n_pad = PIPE2_EPI[(i + j) % 4]
        NT_CASES.append(nt("PIPE2", 0, M, N, K, form, act=1 + (i + j) % 2, n_pad=0 if form == "resf" else n_pad))
# the fp32 mask of the split-operand arithmetic: the weight-stationary kernel has no fp32-mask epilogue, so K = 256 comes here too
for K in (256, 272):
    for j, (M, N) in enumerate(((65, 65), (200, 315), (63, 315), (1, 65))):
        NT_CASES.append(nt("PIPE2", 0, M, N, K, ("maskf", "maskf_res")[j % 2], act=1 + j % 2))

# ---- GENERIC_128x128: gemm_nt_kernel<128, 128>, reachable with the fp32 mask and K < 64 only
for i, K in enumerate((16, 32, 48)):
    for j, M in enumerate((1, 129, 300)):
        for k, N in enumerate((65, 256)):
            NT_CASES.append(nt("GENERIC_128x128", 0, M, N, K, ("maskf", "maskf_res")[(i + j + k) % 2], act=1 + (i + j) % 2,
                               ldc_f32=odd4(65) if (N == 65 and j == 1) else 0))

# ---- GENERIC_128x64 / GENERIC_128x32: gemm_nt_kernel on the narrow layers (W <= 64 / W <= 32), whatever K is: one 16-column step, one
# 64-wide stage and a tail of 48, four whole stages, sixteen stages with a tail of 48
NARROW = (("GENERIC_128x64", ((33, 40), (40, 48), (64, 64))), ("GENERIC_128x32", ((1, 8), (8, 16), (17, 24), (32, 32))))
for kernel, widths in NARROW:
    for i, (N, n_pad) in enumerate(widths):
        for j, K in enumerate((16, 112, 256, 1008)):
            for k, M in enumerate((1, 127, 129, 777)):
                form = (i + j + k) % 3
                if form == 0:
                    NT_CASES.append(nt(kernel, 0, M, N, K, "plain", ldc_f32=odd4(N) if k % 2 else 0))
                elif form == 1:
                    NT_CASES.append(nt(kernel, 0, M, N, K, "biasact", act=1 + (j + k) % 2))
                else:
                    NT_CASES.append(nt(kernel, 0, M, N, K, ("plain", "biasact")[k % 2], act=(k % 2) * (1 + j % 2), n_pad=n_pad))
    for N, _ in widths[::2]:
        for M in (127, 129):
            NT_CASES.append(nt(kernel, 0, M, N, 48, ("maskf", "maskf_res")[M % 2], act=1 + (N % 2)))

# ---- BIG: gemm_nt_big_kernel (128 x 256 tiles, three 64-wide K-stages): >= 4096 rows of a layer >= 512 wide, fewer 256 x 256 tiles than
# the wide kernels ask for.  33 row tiles, the last of 77 rows / of ONE row; 5 stages with a tail of 16, 16 stages with a tail of 48.
for M, N, K, n_pad in ((4096 + 77, 512, 272, 512), (4097, 1000, 1008, 1008)):
    NT_CASES.append(nt("BIG", 0, M, N, K, "full", act=1, n_pad=n_pad))
    NT_CASES.append(nt("BIG", 0, M, N, K, "resf", act=2))
    NT_CASES.append(nt("BIG", 0, M, N, K, "maskb_res", act=1, n_pad=n_pad))
    NT_CASES.append(nt("BIG", 0, M, N, K, "maskf_res", act=2))

# ---- P8 and WIDE: the 256 x 256-tile kernels (the ping-pong kernel of csrc/dhaug_gemm_p8.hip and gemm_nt_wide_kernel, its fallback),
# which a few hundred rows reach through DHAUG_GEMM_WIDE_MIN_TILES=1.  One row, one row short of / beyond a row tile, three row tiles
# with a ragged last one; one whole column tile, a second one of 8 columns, four with a ragged last one.
# P8 cases keep every condition of dhaug_p8_supported() true BY CONSTRUCTION:
#   K >= 128 (two of its 64-wide K-tiles) and K % 8 == 0; N % 8 == 0 and n_pad % 8 == 0; lda, ldb multiples of 8 and >= K (K + 24, K + 16);
#   every pointer 16-byte aligned (a column block starts 8 elements into a 16-byte aligned row; the bias is not moved); the bf16 output's,
#   bf16 residual's and bf16 mask's row strides multiples of 8, the fp32 output's, residual's and mask's multiples of 4 (the defaults of
#   nt() above); no sign-bit mask; operand rows far shorter than 2^31 / 512 elements.
# WIDE cases set DHAUG_GEMM_NOP8, or break exactly ONE of those conditions, named in `why`.
TILES1 = (("DHAUG_GEMM_WIDE_MIN_TILES", "1"),)
P8_K = (144, 272, 1008)                   # (2 K-tiles + 16, 4 + 16, 15 + 48; K = 128 and 256 belong to the weight-stationary kernel)
FORMS4 = ("full", "resf", "maskb_res", "maskf_res")
NOP8 = TILES1 + (("DHAUG_GEMM_NOP8", "1"),)
for i, M in enumerate((1, 255, 257, 520)):
    for j, N in enumerate((256, 264, 1000)):
        for k, form in enumerate(FORMS4):
            K = P8_K[(i + j + k) % 3]
            act = 1 + (i + k) % 2
            assert K >= 128 and K % 8 == 0 and N % 8 == 0          # (the conditions a slip in THIS loop could break)
            NT_CASES.append(nt("P8", 0, M, N, K, form, act=act, n_pad=N, env=TILES1, p8_ok=True))
            # ... and on the fallback kernel
            if form == "full" and i % 2 == 1:
                NT_CASES.append(nt("WIDE", 0, M, N, K, form, act=act, n_pad=N, env=TILES1, p8_ok=False, bias_off=4, why="bias not 16-byte aligned"))
            elif N == 1000 and form in ("resf", "maskf_res") and i % 2 == 0:
                NT_CASES.append(nt("WIDE", 0, M, 1001, K, form, act=act, env=TILES1, p8_ok=False, why="N % 8 != 0"))
            elif (i + j + k) % 3 == 0:
                NT_CASES.append(nt("WIDE", 0, M, N, (80, 96)[(i + k) % 2], form, act=act, n_pad=N, env=TILES1, p8_ok=False, why="K < 128: below two K-tiles"))
            else:
                NT_CASES.append(nt("WIDE", 0, M, N, K, form, act=act, n_pad=N, env=NOP8, p8_ok=True))
# the last column tile lies wholly in the pad: columns 256 .. 263 of a 250-wide layer are zeros written without a weight row to read
for M in (255, 520):
    NT_CASES.append(nt("WIDE", 0, M, 250, 272, "full", act=1, n_pad=264, env=TILES1, p8_ok=False, why="N % 8 != 0"))
NT_CASES.append(nt("P8", 0, 257, 256, 144, "plain", n_pad=264, env=TILES1, p8_ok=True, why="second column tile wholly in the pad"))
NT_CASES.append(nt("WIDE", 0, 257, 256, 144, "plain", n_pad=264, env=NOP8, p8_ok=True, why="second column tile wholly in the pad"))
# a wide layer below the batch the big tiles ask for, with the big-tile kernels switched off altogether: the 64 x 64 tiles again
NT_CASES.append(nt("PIPE2", 0, 520, 1000, 1008, "full", act=1, n_pad=1008, env=TILES1 + (("DHAUG_GEMM_NOBIG", "1"),)))

assert len(set(c.ident for c in NT_CASES)) == len(NT_CASES), "case ids must be unique"
assert all(c.M <= 4200 and c.W <= 1008 and c.K <= 1008 for c in NT_CASES)


@dataclass(frozen=True)
class TnCase:
    M: int
    N1: int
    N2: int
    kernel: str                          # the TnKernel this launch is meant to reach
    colsum_rows: int                     # the row-limited bias sum: a multiple of 128 below M
    why: str = ""

    @property
    def ident(self):
        return "%s-%dx%dx%d" % (self.kernel, self.M, self.N1, self.N2)


# Each TN case is run plain, with `accumulate`, with `colsum`, and with `colsum_rows`.  tn_route: gemm_tn64_kernel takes whole 128-row
# stages, at least four of them, and ragged widths from sixteen stages on.
TN_CASES = [
    TnCase(512, 64, 64, "TN64", 256, "four stages: the minimum"),
    TnCase(512, 256, 256, "TN64", 384, "four stages, sixteen output tiles"),
    TnCase(384, 64, 64, "TN_GENERIC", 128, "three stages: one short of the minimum"),
    TnCase(1920, 100, 100, "TN_GENERIC", 896, "fifteen stages, ragged widths: one short of the rule"),
    TnCase(2048, 100, 100, "TN64", 1024, "sixteen stages, ragged widths"),
    TnCase(2048, 1, 104, "TN64", 1920, "sixteen stages, a single column against a ragged second tile"),
    TnCase(640, 256, 48, "TN_GENERIC", 256, "five stages, a width below one tile"),
]
assert all(c.colsum_rows % 128 == 0 and 0 < c.colsum_rows < c.M for c in TN_CASES)
