"""DOF angle distributions without a GPU: the numpy restatement (tests/dof_util.py) on hand cases, every refusal of the two
entries through the binding and of ops / DofDistribution, limits_from on synthetic counts, the monitor's schedule and its
default (off), and the per-value arithmetic of csrc/dhaug_dof_math.h compiled for the host as a stand-alone program under
AddressSanitizer + UBSan (tests/dofcheck)."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dof_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def pkg():
    import dhaug_amd
    from dhaug_amd import ops
    from dhaug_amd.utils import dof_stats
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model as fkm
    return argparse.Namespace(ops=ops, lib=dhaug_amd._lib, S=dof_stats, fkm=fkm)


def test_restatement_on_hand_cases():
    cases = [(-0.5, 180, False), (0.999, 180, False), (-1.0, 179, False), (180.5, 360, False), (181.0, 360, True),
             (-180.9, 0, False), (-181.0, 0, True), (0.0, 180, False), (-0.0, 180, False), (179.99, 359, False),
             (np.inf, 360, True), (-np.inf, 0, True), (1e30, 360, True)]
    b, nan, outside, inf = U.bins_of([c[0] for c in cases])
    assert b.tolist() == [c[1] for c in cases] and outside.tolist() == [c[2] for c in cases] and not nan.any()
    assert inf.tolist() == [np.isinf(c[0]) for c in cases]
    b, nan, outside, inf = U.bins_of([np.nan])
    assert b.tolist() == [-1] and nan.tolist() == [True] and not outside.any() and not inf.any()
    r = U.histogram(np.array([[np.nan, -0.5], [2.5, np.inf], [-0.0, 0.0]], dtype=np.float32))
    assert r["nan"].tolist() == [1, 0] and r["outside"].tolist() == [0, 1] and r["inf"].tolist() == [0, 1]
    assert r["counts"][0, 182] == 1 and r["counts"][0, 180] == 1 and r["counts"][1, 180] == 2 and r["counts"][1, 360] == 1
    assert (r["counts"].sum(axis=1) + r["nan"]).tolist() == [3, 3]
    assert r["sum"].tolist() == [2.5, -0.5] and r["sumsq"].tolist() == [6.25, 0.25]
    assert np.signbit(r["min"][0]) and r["min"][0] == 0 and r["max"][0] == 2.5 and r["min"][1] == -0.5 and np.isinf(r["max"][1])
    keep = U.kept_rows(4, [0.5, 1.0, 1.5, np.nan], 1.0)
    assert keep.tolist() == [True, True, False, False]


def test_header_constants_and_partition(pkg):
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, hdr).group(1))
    L = pkg.lib
    assert (define("DHAUG_DOF_BINS"), define("DHAUG_DOF_MAX_SLOTS"), define("DHAUG_DOF_MAX_PAIRS"), define("DHAUG_DOF_BLOCK"),
            define("DHAUG_DOF_MAX_BLOCKS"), define("DHAUG_DOF_MIN_STEPS")) == (L.DOF_BINS, L.DOF_MAX_SLOTS, L.DOF_MAX_PAIRS,
                                                                               L.DOF_BLOCK, L.DOF_MAX_BLOCKS, L.DOF_MIN_STEPS)
    off = L.dof_record_offsets(37)
    names = ["rows", "skipped", "nan", "outside", "at_lo", "at_hi", "inf", "min", "max", "sum", "sumsq", "counts"]
    assert [off[n] for n in names] == [0, 1] + [2 + 37 * i for i in range(10)] and off["words"] == 2 + 37 * (9 + 361)
    for n in names[2:]:
        m = re.search(r"#define\s+DHAUG_DOF_OFF_%s\(D\)\s+(.+)" % n.upper(), hdr).group(1)
        assert eval(m.replace("(D)", "(37)")) == off[n], n
    for D in (1, 33, 37, 64):                        # the library that is loaded lays the record out as the binding believes
        assert L.dof_record_layout(D) == L.dof_record_offsets(D), D
    with pytest.raises(RuntimeError, match="DHAUG_EINVAL"):
        L.dof_record_layout(65)
    assert L.DOF_WORKSPACE_BYTES == L.DOF_MAX_BLOCKS * 4 * L.DOF_MAX_SLOTS * 8
    assert L.dof_partition(1, 37) == (6, 1, 6) and L.dof_partition(6 * 16 + 1, 37) == (6, 2, 54)
    assert L.dof_partition(512 * 16 * 6 + 1, 37) == (6, 482, 17 * 6) and L.dof_partition(0, 37)[1] == 0


def test_every_error_code_through_the_binding(pkg):
    """all refusals come before any launch, so fake (never dereferenced) device addresses will do"""
    lib = pkg.lib.lib()
    A, R, W, T = 0x10000, 0x20000, 0x30000, 0x40000
    hist = lambda angles=A, rows=8, D=37, pitch=37, res=None, lo=None, hi=None, rec=R, ws=W: lib.dhaug_dof_histogram(
        angles, rows, D, pitch, res, 0.0, lo, hi, 0.0, rec, ws, None)
    pairs_t = ctypes.c_int * 8

    def pair(angles=A, rows=8, D=37, pitch=37, pairs=(8, 3), npairs=None, table=T):
        arr = pairs_t(*(list(pairs) + [0] * (8 - len(pairs))))
        return lib.dhaug_dof_pair_histogram(angles, rows, D, pitch, None, 0.0, arr, len(pairs) // 2 if npairs is None else npairs,
                                            table, None)
    for fn in (hist, pair):
        assert fn(rows=-1) == EINVAL and fn(D=0) == EINVAL and fn(D=65) == EINVAL and fn(pitch=36) == EINVAL
        assert fn(angles=None) == EINVAL
        assert fn(rows=1 << 31) == EUNSUPPORTED
        assert fn(rows=0, angles=None) == 0                       # a no-op: nothing is launched, nothing is read
    assert hist(rec=None) == EINVAL and hist(ws=None) == EINVAL
    assert hist(lo=0x50000) == EINVAL and hist(hi=0x50000) == EINVAL
    assert hist(rec=R + 4) == EALIGN and hist(ws=W + 4) == EALIGN
    assert pair(table=None) == EINVAL and pair(table=T + 4) == EALIGN
    assert pair(pairs=(8, 37)) == EINVAL and pair(pairs=(-1, 3)) == EINVAL and pair(D=33, pairs=(0, 33)) == EINVAL
    assert pair(npairs=5) == EINVAL and pair(npairs=-1) == EINVAL
    assert pair(pairs=(), npairs=0) == 0                          # no pair: a no-op


def test_ops_and_accumulator_refusals(pkg):
    ops, S = pkg.ops, pkg.S
    off = pkg.lib.dof_record_offsets(37)
    a, rec = torch.zeros(4, 37), torch.zeros(off["words"], dtype=torch.int64)
    table = torch.zeros(1, 361, 361, dtype=torch.int64)
    lo = torch.zeros(37)
    for fn in (lambda: ops.dof_record(0), lambda: ops.dof_record(65),
               lambda: ops.dof_histogram(torch.zeros(4, 37, 1), rec), lambda: ops.dof_histogram(torch.zeros(4, 65), rec),
               lambda: ops.dof_histogram(a, rec[:-1]), lambda: ops.dof_histogram(a, rec.double()),
               lambda: ops.dof_histogram(a, rec, lo=lo), lambda: ops.dof_histogram(a, rec, lo=lo, hi=lo[:36]),
               lambda: ops.dof_histogram(a, rec, tol=-1.0), lambda: ops.dof_histogram(a, rec, residual=torch.zeros(4)),
               lambda: ops.dof_histogram(a, rec, max_residual=1e-4),
               lambda: ops.dof_histogram(a, rec, residual=torch.zeros(3), max_residual=1e-4),
               lambda: ops.dof_pair_histogram(a, [(8, 37)], table), lambda: ops.dof_pair_histogram(a, [(0, 1)] * 5, table),
               lambda: ops.dof_pair_histogram(a, [(0, 1)], table[0]), lambda: ops.dof_pair_histogram(a, [(0, 1)], table.int()),
               lambda: ops.dof_pair_histogram(a, [3], table),
               lambda: S.DofDistribution(D=0), lambda: S.DofDistribution(D=65), lambda: S.DofDistribution(pairs=((0, 37),)),
               lambda: S.DofDistribution(pairs=(3,)), lambda: S.DofDistribution(tol=-0.5),
               lambda: S.DofDistribution(limits=([0.0] * 37, [0.0] * 36)), lambda: S.DofDistribution(limits=([1.0] * 37, [0.0] * 37)),
               lambda: S.DofDistribution(limits=[0.0] * 37),
               lambda: S.DofMonitor(None), lambda: S.limits_from_counts(np.zeros((2, 361)), 0.0),
               lambda: S.limits_from_counts(np.zeros((2, 360)))):
        with pytest.raises(ValueError):
            fn()
    # what passes the host checks then asks for GPU tensors, as every op does
    for fn in (lambda: ops.dof_histogram(a, rec), lambda: ops.dof_pair_histogram(a, [(8, 3)], table)):
        with pytest.raises(RuntimeError, match="needs GPU tensors"):
            fn()
    fk = pkg.fkm.Forward_Kinematics_DH_Model(argparse.Namespace(batch_size=2, random_seed=0), ["S1"], None)
    with pytest.raises(ValueError):
        fk.dof_distribution(torch.zeros(4, 16, 3), into="no accumulator")


def test_limits_from_synthetic_counts(pkg):
    F = pkg.S.limits_from_counts
    c = np.zeros((6, 361), dtype=np.int64)
    c[0, 200] = 7                                   # one bin: [20, 21)
    c[1, 100], c[1, 300] = 5, 5                     # two separated bins: both stay at any coverage above one half
    c[2, 180] = 3                                   # bin 180 is (-1, 1)
    c[3, 170:191] = 1000                            # a plateau with one stray count far out on either side
    c[3, 10], c[3, 350] = 1, 1
    c[4, 0], c[4, 360] = 2, 2                       # the end bins
    lo, hi = F(c, 0.999)
    assert (lo[0], hi[0]) == (20.0, 21.0) and (lo[1], hi[1]) == (-81.0, 121.0) and (lo[2], hi[2]) == (-1.0, 1.0)
    assert (lo[3], hi[3]) == (-11.0, 11.0) and (lo[4], hi[4]) == (-181.0, 181.0) and (lo[5], hi[5]) == (0.0, 0.0)
    big = np.zeros((1, 361), dtype=np.int64)        # exact at totals where coverage * total is not a double
    big[0, 100], big[0, 200], big[0, 300] = 1, 2 ** 60, 1
    assert F(big, 1.0) == ([-81.0], [121.0]) and F(big, 0.5) == ([20.0], [21.0])
    lo, hi = F(c, 1.0)                              # coverage 1.0 drops nothing
    assert (lo[3], hi[3]) == (-171.0, 171.0) and (lo[1], hi[1]) == (-81.0, 121.0)
    assert all(a <= b for a, b in zip(lo, hi)) and len(lo) == 6
    assert [pkg.S.bin_edges(b) for b in (0, 179, 180, 181, 360)] == [(-181, -180), (-2, -1), (-1, 1), (1, 2), (180, 181)]


def test_monitor_schedule_and_defaults(pkg, monkeypatch):
    class Dist(pkg.S.DofDistribution):
        def __init__(self):                          # (no device: the schedule alone)
            pass
    m = pkg.S.DofMonitor(Dist(), every=500)
    assert [n for n in range(1, 1003) if m.due(n)] == [1, 501, 1001] and not m.due(0)
    assert all(pkg.S.DofMonitor(Dist(), every=1).due(n) for n in range(1, 5))
    with pytest.raises(ValueError):
        pkg.S.DofMonitor(Dist(), every=0)
    monkeypatch.delenv("DHAUG_DOF_MONITOR", raising=False)
    assert not pkg.S.monitor_enabled(argparse.Namespace()) and pkg.S.monitor_enabled(argparse.Namespace(dof_monitor=True))
    monkeypatch.setenv("DHAUG_DOF_MONITOR", "1")
    assert pkg.S.monitor_enabled(argparse.Namespace())


def test_monitor_is_off_on_fresh_generators_and_factories(pkg, monkeypatch):
    from dhaug_amd.models_Fk_GAN import Fk_generator, model_fk_gan_train as T
    monkeypatch.delenv("DHAUG_DOF_MONITOR", raising=False)
    args = argparse.Namespace(batch_size=8, random_seed=0, GAN_OUTPUT_DIM=35, GAN_whether_use_preAngle=True, Gen_DenseDim=32,
                              bone_len_scaler="different", whether_use_RT=True)
    assert Fk_generator.Fk_Generator(None, args, "cpu").dof_monitor is None
    assert Fk_generator.Video_Fk_Generator(3, None, args, "cpu").dof_monitor is None
    # what the factories do once the models are built, on a stand-in dictionary: building the models needs a GPU, and
    # tests/test_gpu_dof.py::test_factories_attach_the_monitor_only_when_asked calls both factories themselves
    class G:
        dof_monitor = None
    d = T._with_dof_monitor(args, "cpu", {"model_G": G()})
    assert d["model_G"].dof_monitor is None and "dof_distribution" not in d


def test_figure_is_written_only_when_asked(tmp_path):
    """the drawing half of the three drop-ins: <checkpoint>/tmp/<name>.jpg when args.record_all_picture is true, nothing otherwise.
    matplotlib (with Pillow for the .jpg) is an OPTIONAL dependency of the feature -- without it the functions return their tables
    and draw nothing, which test_without_matplotlib_nothing_is_drawn checks on every machine -- so only this test needs it."""
    pytest.importorskip("matplotlib")
    pytest.importorskip("PIL")
    from dhaug_amd.models_Fk_GAN import special_operate as sp
    table = np.arange(361.0 * 4).reshape(4, 361)
    draw = lambda ax, plt: ax.matshow(table, cmap=plt.cm.Blues)
    sp._dof_figure(argparse.Namespace(record_all_picture=False, checkpoint=str(tmp_path)), "off", draw)
    sp._dof_figure(argparse.Namespace(checkpoint=str(tmp_path)), "absent", draw)
    assert not list(tmp_path.iterdir())
    sp._dof_figure(argparse.Namespace(record_all_picture=True, checkpoint=str(tmp_path)), "on", draw)
    assert [p.name for p in (tmp_path / "tmp").iterdir()] == ["on.jpg"] and (tmp_path / "tmp" / "on.jpg").stat().st_size > 0


def test_without_matplotlib_nothing_is_drawn(tmp_path, monkeypatch):
    """`import matplotlib` failing (None in sys.modules raises ImportError) is not an error: no file, no exception"""
    from dhaug_amd.models_Fk_GAN import special_operate as sp
    for name in [n for n in sys.modules if n == "matplotlib" or n.startswith("matplotlib.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "matplotlib", None)
    called = []
    sp._dof_figure(argparse.Namespace(record_all_picture=True, checkpoint=str(tmp_path)), "none", lambda ax, plt: called.append(1))
    assert not called and not list(tmp_path.iterdir())


def test_host_program_under_sanitizers():
    """tests/dofcheck: dhaug_dof_math.h compiled for the host with -fsanitize=address,undefined as a program of its own: every
    fp32 value within 4 ulp of the integers -182..182, zeros, denormals, +-1e30, +-inf and NaN get the restatement's bin and
    flags, and no float is converted to int out of range"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    exe = ge.build_dofcheck_sanitized(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"^checked (\d+) values, 0 mismatches$", r.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 365 * 9, r.stdout[-2000:]
