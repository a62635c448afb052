"""GPU tests of the FK and generator-tail kernels (csrc/dhaug_fk.hip) through the C-ABI, with buffers of their own: every output has
3 extra rows of poison behind it that must be found untouched.  Accuracy is measured per column (tests/fk_tail_util.py) on one batch
of 193 poses -- three full tiles and a one-row tile -- against the CPU oracle in fp64, with the oracle in fp32 as the yardstick;
raggedness, a second trip of the tile loops and the in-kernel Philox draw are then tested by bit-equality.

    dhaug_fk_forward                  test_fk_forward_null_root_per_column, test_fk_forward_second_trip
    dhaug_fk_backward                 test_fk_backward_per_column, test_fk_backward_second_trip
    dhaug_gen_tail_forward            test_gen_tail_forward_saturated_rows, test_gen_tail_second_trip
    dhaug_gen_tail_backward           test_gen_tail_backward_per_column, test_gen_tail_second_trip
    dhaug_gen_tail_forward_critics    test_gen_tail_forward_saturated_rows, test_inputs_bf16_is_the_rounded_fp32_output,
                                      test_in_kernel_jitter_bits, test_gen_tail4_second_trip
The multi-pass sizes come from the binding's mirror of the grid caps (tests/test_cpu_boundary.py pins it to the header)."""
import os
import sys

import numpy as np
import pytest
import torch

import fk_tail_util as U
import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
POISON = 7.5e37
EXTRA = 3
N0 = 193
QUAT = [0.1407056450843811, -0.1500701755285263, -0.755240797996521, 0.6223280429840088]
TRANS = [1.841107, 4.955284, 1.563445]
CAM9 = [2.29, 2.287, 0.0251, 0.0289, -0.207, 0.2478, -0.00307, -0.00097, -0.00142]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    dhaug_amd._lib.lib()
    return dhaug_amd._lib


def stream():
    return torch.cuda.current_stream().cuda_stream or None


class Out:
    """an (N, W) output with EXTRA poisoned rows behind it (7.5e37; NaN for bf16)"""

    def __init__(self, N, W, dtype=torch.float32):
        self.N, self.dtype = N, dtype
        self.full = torch.full((N + EXTRA, W), float("nan") if dtype == BF16 else POISON, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return self.full.data_ptr()

    def rows(self):
        tail = self.full[self.N:]
        ok = torch.isnan(tail).all() if self.dtype == BF16 else (tail == POISON).all()
        assert bool(ok), "rows behind the output were written"
        return self.full[:self.N]


def ptr(t, row=0):
    return None if t is None else t.data_ptr() + row * t.stride(0) * t.element_size()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ---- the five entry points on device buffers; `row` = first row of the inputs, N rows from there ----------------------------------
def fk_forward(L, a, bl, rt, N, joints, row=0):
    out = Out(N, joints * 3)
    L.call("dhaug_fk_forward", ptr(a, row), ptr(bl, row), ptr(rt, row), out.ptr, N, joints, stream())
    return out.rows()


def fk_backward(L, a, bl, g, N, row=0):
    ga, gb, gr = Out(N, 37), Out(N, 15), Out(N, 3)
    L.call("dhaug_fk_backward", ptr(a, row), ptr(bl, row), ptr(g, row), ga.ptr, gb.ptr, gr.ptr, N, stream())
    return ga.rows(), gb.rows(), gr.rows()


def tail_forward(L, head, bl, sc, N, pre, row=0):
    fake, ang = Out(N, 48), Out(N, 37)
    L.call("dhaug_gen_tail_forward", ptr(head, row), ptr(bl, row), ptr(sc, row), fake.ptr, ang.ptr, N, int(pre), stream())
    return fake.rows(), ang.rows()


def tail_backward(L, head, bl, sc, g, N, pre, row=0):
    gh = Out(N, 35)
    L.call("dhaug_gen_tail_backward", ptr(head, row), ptr(bl, row), ptr(sc, row), ptr(g, row), gh.ptr, N, int(pre), stream())
    return gh.rows()


def critics(L, head, bl, sc, N, pre, camera=False, rng=None, want=("centered", "kcs", "proj2d", "scaler_out"), bf16=False, row=0):
    """dhaug_gen_tail_forward_critics: a dict of the outputs that were asked for (proj2d needs the camera, scaler_out a draw)"""
    import ctypes
    idt = BF16 if bf16 else torch.float32
    o = {"fake": Out(N, 48)}
    if "centered" in want:
        o["centered"] = Out(N, 48, idt)
    if "kcs" in want:
        o["kcs"] = Out(N, 32, BF16)
    q = t = c = None
    if camera and "proj2d" in want:
        o["proj2d"] = Out(N, 32, idt)
        q, t, c = (ctypes.c_float * 4)(*QUAT), (ctypes.c_float * 3)(*TRANS), (ctypes.c_float * 9)(*CAM9)
    if rng is not None and "scaler_out" in want:
        o["scaler_out"] = Out(N, 8)
    p = lambda k: o[k].ptr if k in o else None
    seed, offset = (0, 0) if rng is None else rng
    L.call("dhaug_gen_tail_forward_critics", ptr(head, row), ptr(bl, row), ptr(sc, row), o["fake"].ptr, p("centered"), p("kcs"), q, t, c,
           p("proj2d"), int(rng is not None), seed, offset, p("scaler_out"), N, int(pre), int(bf16), stream())
    return {k: v.rows() for k, v in o.items()}


# ---- the batch of 193 ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fk_batch():
    a, bl, rt = GU.synth_fk_inputs(N0, 41)
    g = torch.randn(N0, 48, generator=torch.Generator().manual_seed(42))
    zero = torch.zeros_like(rt)
    return dict(a=a, bl=bl, g=g, r64=U.fk_oracle(a, bl, zero, g, torch.float64), r32=U.fk_oracle(a, bl, zero, g, torch.float32),
                dev=tuple(t.cuda() for t in (a, bl, g)))


@pytest.fixture(scope="module")
def tail_batch():
    head, bl, sc, g = U.tail_inputs(N0, 43)
    return dict(head=head, bl=bl, sc=sc, g=g, dev=tuple(t.cuda() for t in (head, bl, sc, g)), oracle={})


def tail_ref(tb, pre, with_scaler):
    """(fp64, fp32) oracle runs of the batch, computed once per configuration"""
    key = (bool(pre), bool(with_scaler))
    if key not in tb["oracle"]:
        sc = tb["sc"] if with_scaler else None
        tb["oracle"][key] = tuple(U.tail_oracle(tb["head"], tb["bl"], sc, tb["g"], pre, dt) for dt in (torch.float64, torch.float32))
    return tb["oracle"][key]


# ---- a. dhaug_fk_backward per column -----------------------------------------------------------------------------------------------
def test_fk_backward_per_column(L, fk_batch):
    a, bl, g = fk_batch["dev"]
    r64, r32 = fk_batch["r64"], fk_batch["r32"]
    got = fk_backward(L, a, bl, g, N0)
    assert U.dead_columns(r64[1]) == U.FK_DEAD_ANGLE_COLUMNS
    for name, t, i in (("fk_backward_grad_angles", got[0], 1), ("fk_backward_grad_bone_len", got[1], 2), ("fk_backward_grad_root", got[2], 3)):
        U.check_columns(name, t, r64[i], r32[i])
    assert bool((got[0][:, U.FK_DEAD_ANGLE_COLUMNS] == 0).all())
    again = fk_backward(L, a, bl, g, N0)
    assert all(same_bits(x, y) for x, y in zip(got, again))
    for n in (1, 63, 64, 65):                                  # poses are independent lanes: a prefix of the batch gives the same bits
        part = fk_backward(L, a, bl, g, n)
        assert all(same_bits(x, y[:n]) for x, y in zip(part, got)), n


# ---- b. dhaug_gen_tail_backward per column -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [1, 0])
@pytest.mark.parametrize("with_scaler", [True, False])
def test_gen_tail_backward_per_column(L, tail_batch, pre, with_scaler):
    """allowance 4 x 1.2e-7 for tanh_fast (tests/fk_tail_util.py).  FIGURES of the first run on an MI355X are in DESIGN.md."""
    head, bl, sc, g = tail_batch["dev"]
    sc = sc if with_scaler else None
    r64, r32 = tail_ref(tail_batch, pre, with_scaler)
    assert U.dead_columns(r64[2]) == U.HEAD_DEAD_COLUMNS
    got = tail_backward(L, head, bl, sc, g, N0, pre)
    U.check_columns("gen_tail_backward_pre%d_%s" % (pre, "scaler" if with_scaler else "noscaler"), got, r64[2], r32[2], U.TANH_ALLOWANCE)
    assert bool((got[:, U.HEAD_DEAD_COLUMNS] == 0).all())
    assert same_bits(got, tail_backward(L, head, bl, sc, g, N0, pre))
    for n in (1, 63, 65):
        assert same_bits(tail_backward(L, head, bl, sc, g, n, pre), got[:n]), n


# ---- c. forwards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joints", [16, 32])
def test_fk_forward_null_root_per_column(L, fk_batch, joints):
    a, bl, _ = fk_batch["dev"]
    out = fk_forward(L, a, bl, None, N0, joints)
    ref64, ref32 = fk_batch["r64"][0], fk_batch["r32"][0]
    if joints == 32:
        from oracle import dhaug_oracle as O
        zero = torch.zeros(N0, 3)
        ref64 = O.fk_forward32(fk_batch["a"].double(), fk_batch["bl"].double(), zero.double()).reshape(N0, 96)
        ref32 = O.fk_forward32(fk_batch["a"], fk_batch["bl"], zero).reshape(N0, 96)
        o3 = out.reshape(N0, 32, 3)
        never = [j for j in range(32) if j not in O.H36M_32_TO_16 and j != 14]
        assert len(never) == 15 and bool((o3[:, never] == 0).all())                      # rows the reference never writes = the root
        assert same_bits(o3[:, 14], o3[:, 15])
        assert same_bits(o3[:, O.H36M_32_TO_16].reshape(N0, 48), fk_forward(L, a, bl, None, N0, 16))
    U.check_columns("fk_forward_null_root_%d" % joints, out, ref64, ref32)
    assert bool((out[:, :3] == 0).all())                                                 # joint 0 is the root
    zero_root = torch.zeros(N0, 3, device="cuda")
    assert same_bits(out, fk_forward(L, a, bl, zero_root, N0, joints))


@pytest.fixture(scope="module")
def saturated():
    """the tail batch with rows of heads +-20, +-100 (tanh exactly +-1: both ends of every joint range, root +-10) and +-inf, the
    infinite rows sharing bone lengths and jitter with the +-100 rows"""
    head, bl, sc, _ = U.tail_inputs(N0, 43)
    for r, v in ((10, 20.0), (11, -20.0), (12, 100.0), (13, -100.0), (14, float("inf")), (15, -float("inf")), (192, 100.0)):
        head[r] = v
    bl[14], sc[14], bl[15], sc[15] = bl[12], sc[12], bl[13], sc[13]
    return dict(head=head, bl=bl, sc=sc, dev=tuple(t.cuda() for t in (head, bl, sc)))


@pytest.mark.parametrize("pre", [1, 0])
def test_gen_tail_forward_saturated_rows(L, saturated, pre):
    head, bl, sc = saturated["dev"]
    zero_g = torch.zeros(N0, 48)
    ref_fake, ref_ang, _ = U.tail_oracle(saturated["head"], saturated["bl"], saturated["sc"], zero_g, pre, torch.float64)
    assert bool(torch.isfinite(ref_fake).all())
    fake, ang = tail_forward(L, head, bl, sc, N0, pre)
    assert bool(torch.isfinite(fake).all()) and bool(torch.isfinite(ang).all())
    da = (ang.double().cpu() - ref_ang).abs().max().item()
    df = (fake.double().cpu() - ref_fake).abs().max().item()
    print("FIGURE gen_tail_forward_pre%d angles_out %.4g deg (bound 2e-4), fake16 %.4g m (bound 1e-5)" % (pre, da, df))
    assert da <= 2e-4 and df <= 1e-5
    assert same_bits(fake[14], fake[12]) and same_bits(fake[15], fake[13]) and same_bits(ang[14], ang[12]) and same_bits(ang[15], ang[13])
    if pre:                                                    # both ends of every joint range, exactly
        from oracle import dhaug_oracle as O
        hi, lo = torch.tensor(O.ANGLE_HI, dtype=torch.float32), torch.tensor(O.ANGLE_LO, dtype=torch.float32)
        assert bool(torch.equal(ang[12].cpu(), hi)) and bool(torch.equal(ang[13].cpu(), lo)) and bool(torch.equal(ang[10].cpu(), hi))
    # the four-wave kernel on the same rows: the only place its unguarded sincos meets |angle| = 360 degrees
    for camera in (False, True):
        c = critics(L, head, bl, sc, N0, pre, camera=camera)
        d4 = (c["fake"] - fake).abs().max().item()
        print("FIGURE gen_tail_forward_critics_pre%d fake16 against the one-wave kernel %.4g (bound 1e-6)" % (pre, d4))
        assert bool(torch.isfinite(c["fake"]).all()) and d4 <= 1e-6
        assert same_bits(c["fake"][14], c["fake"][12]) and same_bits(c["fake"][15], c["fake"][13])
        assert (c["fake"].double().cpu() - ref_fake).abs().max().item() <= 1e-5


# ---- d. inputs_bf16 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("N", [1, 63, 261])
def test_inputs_bf16_is_the_rounded_fp32_output(L, N, camera):
    head, bl, sc, _ = (t.cuda() for t in U.tail_inputs(N, 50 + N))
    f32 = critics(L, head, bl, sc, N, 1, camera=camera)
    b16 = critics(L, head, bl, sc, N, 1, camera=camera, bf16=True)
    assert set(f32) == set(b16) == {"fake", "centered", "kcs"} | ({"proj2d"} if camera else set())
    assert b16["centered"].dtype == BF16 and same_bits(b16["centered"], f32["centered"].to(BF16))
    assert same_bits(b16["kcs"], f32["kcs"]) and same_bits(b16["fake"], f32["fake"])
    assert same_bits(f32["centered"], f32["fake"] - f32["fake"][:, :3].repeat(1, 16))
    if camera:
        assert b16["proj2d"].dtype == BF16 and same_bits(b16["proj2d"], f32["proj2d"].to(BF16))
    for mode, full in ((False, f32), (True, b16)):
        for drop in ("centered", "kcs", "proj2d"):             # each optional output passed NULL once: the others do not change
            want = tuple(k for k in ("centered", "kcs", "proj2d") if k != drop)
            part = critics(L, head, bl, sc, N, 1, camera=camera, want=want, bf16=mode)
            assert drop not in part
            assert all(same_bits(part[k], full[k]) for k in part), (mode, drop)


# ---- e. Philox bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,offset", [(0, 0), (1234, 16), (2 ** 64 - 1, 2 ** 32 - 1), (0x0123456789abcdef, 2 ** 40 + 8)])
def test_in_kernel_jitter_bits(L, seed, offset):
    """N = 261: four full tiles and a five-row tile, so every wave takes every role and one tile is ragged"""
    N = 261
    head, bl, _, _ = (t.cuda() for t in U.tail_inputs(N, 60))
    drawn = critics(L, head, bl, None, N, 1, camera=True, rng=(seed, offset))
    ref = torch.from_numpy(U.jitter_reference(seed, offset, range(N)))
    assert same_bits(drawn["scaler_out"].cpu(), ref)
    explicit = critics(L, head, bl, drawn["scaler_out"].contiguous(), N, 1, camera=True)
    assert all(same_bits(drawn[k], explicit[k]) for k in explicit)
    silent = critics(L, head, bl, None, N, 1, camera=True, rng=(seed, offset), want=("centered", "kcs", "proj2d"))
    assert "scaler_out" not in silent and all(same_bits(silent[k], drawn[k]) for k in silent)
    plain = critics(L, head, bl, None, N, 1, camera=True)
    assert not same_bits(plain["fake"], drawn["fake"])         # (the draw was used)


# ---- f. past one grid pass ---------------------------------------------------------------------------------------------------------
def sampled_rows(N):
    """400 rows: the last 101 (the second trip's ragged end), 99 around the end of the first pass, 200 spread over the batch"""
    g = torch.Generator().manual_seed(N)
    first = N - 101 - (N - 101) % 64                           # rows of the second trip start here (N = cap * 64 + 101)
    rows = set(range(N - 101, N)) | set(range(first - 49, first + 50))
    for r in torch.randperm(N, generator=g).tolist():
        if len(rows) == 400:
            break
        rows.add(r)
    return sorted(rows)


@pytest.fixture(scope="module")
def big(L):
    """inputs for N1 = FK_MAX_BLOCKS * 64 + 101 poses, generated once on the CPU: the four-wave entry uses the first N4 of them"""
    N1, N4 = L.FK_MAX_BLOCKS * 64 + 101, L.GEN_TAIL4_MAX_BLOCKS * 64 + 101
    assert N4 < N1
    g = torch.Generator().manual_seed(71)
    host = dict(a=(torch.rand(N1, 37, generator=g) * 2 - 1) * 180.0, bl=torch.rand(N1, 15, generator=g) * 0.4 + 0.1,
                rt=torch.randn(N1, 3, generator=g).clamp(-10, 10), head=torch.randn(N1, 35, generator=g),
                sc=torch.randint(-200, 200, (N1, 8), generator=g).float() / 1000.0, g=torch.randn(N1, 48, generator=g))
    host["head"][::7] *= 4.0
    return dict(N1=N1, N4=N4, host=host, dev={k: v.cuda() for k, v in host.items()}, rows1=sampled_rows(N1), rows4=sampled_rows(N4))


def two_calls(fn, N, cap):
    """fn(n, row) -> tensor or tuple of tensors: the full call, and the two calls on [0, cap * 64) and [cap * 64, N) joined"""
    tup = lambda x: x if isinstance(x, tuple) else (x,)
    full = tup(fn(N, 0))
    lo, hi = tup(fn(cap * 64, 0)), tup(fn(N - cap * 64, cap * 64))
    return full, tuple(torch.cat([x, y]) for x, y in zip(lo, hi))


@pytest.mark.parametrize("joints", [16, 32])
def test_fk_forward_second_trip(L, big, joints):
    d, N, cap = big["dev"], big["N1"], L.FK_MAX_BLOCKS
    assert (N + 63) // 64 > cap and N - cap * 64 == 101
    full, parts = two_calls(lambda n, row: fk_forward(L, d["a"], d["bl"], d["rt"], n, joints, row), N, cap)
    assert same_bits(full[0], parts[0])
    if joints == 16:
        rows, h = big["rows1"], big["host"]
        r64 = U.fk_oracle(h["a"][rows], h["bl"][rows], h["rt"][rows], torch.zeros(len(rows), 48), torch.float64)[0]
        assert (full[0][rows].double().cpu() - r64).abs().max().item() <= 4e-6              # the bound of test_fk_forward_ragged_sizes


def test_fk_backward_second_trip(L, big):
    d, N, cap = big["dev"], big["N1"], L.FK_MAX_BLOCKS
    full, parts = two_calls(lambda n, row: fk_backward(L, d["a"], d["bl"], d["g"], n, row), N, cap)
    assert all(same_bits(x, y) for x, y in zip(full, parts))
    rows, h = big["rows1"], big["host"]
    r64 = U.fk_oracle(h["a"][rows], h["bl"][rows], h["rt"][rows], h["g"][rows], torch.float64)
    for got, ref in zip(full, r64[1:]):
        assert (got[rows].double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()   # the bound of test_fk_backward


@pytest.mark.parametrize("pre", [1, 0])
@pytest.mark.parametrize("with_scaler", [True, False])
def test_gen_tail_second_trip(L, big, pre, with_scaler):
    d, N, cap = big["dev"], big["N1"], L.FK_MAX_BLOCKS
    sc = d["sc"] if with_scaler else None
    full, parts = two_calls(lambda n, row: tail_forward(L, d["head"], d["bl"], sc, n, pre, row), N, cap)
    assert all(same_bits(x, y) for x, y in zip(full, parts))
    gfull, gparts = two_calls(lambda n, row: tail_backward(L, d["head"], d["bl"], sc, d["g"], n, pre, row), N, cap)
    assert same_bits(gfull[0], gparts[0])
    rows, h = big["rows1"], big["host"]
    ref = U.tail_oracle(h["head"][rows], h["bl"][rows], h["sc"][rows] if with_scaler else None, h["g"][rows], pre, torch.float64)
    assert (full[0][rows].double().cpu() - ref[0]).abs().max().item() <= 1e-5
    assert (full[1][rows].double().cpu() - ref[1]).abs().max().item() <= 2e-4
    assert (gfull[0][rows].double().cpu() - ref[2]).abs().max().item() <= 1e-4 * ref[2].abs().max().item()


@pytest.mark.parametrize("pre", [1, 0])
def test_gen_tail4_second_trip(L, big, pre):
    d, N, cap = big["dev"], big["N4"], L.GEN_TAIL4_MAX_BLOCKS
    assert (N + 63) // 64 > cap and N - cap * 64 == 101
    keys = ("fake", "centered", "kcs", "proj2d")
    rows, h = big["rows4"], big["host"]
    explicit = None
    for sc in (d["sc"], None):
        for bf16 in ((False, True) if sc is not None else (False,)):
            full, parts = two_calls(lambda n, row: tuple(critics(L, d["head"], d["bl"], sc, n, pre, camera=True, bf16=bf16, row=row)[k]
                                                         for k in keys), N, cap)
            assert all(same_bits(x, y) for x, y in zip(full, parts)), (sc is None, bf16)
            if sc is not None and not bf16:
                explicit = full
            if not bf16:
                ref = U.tail_oracle(h["head"][rows], h["bl"][rows], h["sc"][rows] if sc is not None else None, torch.zeros(len(rows), 48),
                                    pre, torch.float64)
                assert (full[0][rows].double().cpu() - ref[0]).abs().max().item() <= 1e-5
    # draw mode: the counter is the global pose index; fed back as an explicit scaler the draw gives the same poses
    seed, offset = 0x0123456789abcdef, 2 ** 40 + 8
    drawn = critics(L, d["head"], d["bl"], None, N, pre, camera=True, rng=(seed, offset))
    assert same_bits(drawn["scaler_out"][rows].cpu(), torch.from_numpy(U.jitter_reference(seed, offset, rows)))
    again = critics(L, d["head"], d["bl"], drawn["scaler_out"], N, pre, camera=True)
    assert all(same_bits(drawn[k], again[k]) for k in keys)
    assert not same_bits(drawn["fake"], explicit[0])
