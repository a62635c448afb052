"""CPU-side checks of the replayable posenet step: the new entry points (the device-stream BatchNorm launches, the 64-bit add, Adam
with the learning rate in device memory) return their documented codes for bad arguments before any launch, their ctypes
signatures are the header's, and StepRunner(graph=True) refuses what it cannot capture without touching a GPU."""
import argparse
import ctypes
import os
import re
import sys

import pytest
import torch

import posenet_util as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, EUNSUP = -1, -2, -3
NEW = ("dhaug_bn_act_forward_dr", "dhaug_bn_act_backward_partials_dr", "dhaug_bn_act_backward_dr", "dhaug_u64_add",
       "dhaug_adam_clip_step_lr")


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def host(built):
    """valid HOST addresses: a call that got as far as a launch would come back with a HIP error, not with one of the codes"""
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    return dict(keep=buf, L=built._lib.lib(), a=ctypes.c_void_p(base), b=ctypes.c_void_p(base + 8192), c=ctypes.c_void_p(base + 16384),
                cell=ctypes.c_void_p(base + 24576), odd=ctypes.c_void_p(base + 4))


def test_dr_forward_argument_errors(host):
    L, a, b, c, cell, odd = (host[k] for k in ("L", "a", "b", "c", "cell", "odd"))

    def fwd(z=a, zb=0, ld=16, res=None, ldr=0, g=b, bt=b, mean=b, rstd=b, ws=c, rm=None, rv=None, nbt=None, mom=0.1, eps=1e-5,
            p=0.0, rng=cell, yb=None, ldyb=0, yf=c, ldyf=16, M=4, C=16):
        return L.dhaug_bn_act_forward_dr(z, zb, ld, res, ldr, g, bt, mean, rstd, ws, rm, rv, nbt, mom, eps, p, rng, 4, yb, ldyb, yf,
                                         ldyf, M, C, None)

    # the cell: required exactly when there is dropout
    assert fwd(p=0.25, rng=None) == EINVAL
    assert fwd(p=0.25, rng=odd) == EALIGN
    assert fwd(p=0.0, rng=None, M=0) == 0 and fwd(p=0.25, rng=None, M=0) == EINVAL      # (checked before the empty batch returns)
    # every other check is dhaug_bn_act_forward's (tests/test_posenet_cpu.py), with and without dropout
    for p in (0.0, 0.25):
        assert fwd(p=p, z=None) == EINVAL and fwd(p=p, g=None) == EINVAL and fwd(p=p, mean=None) == EINVAL and fwd(p=p, yf=None) == EINVAL
        assert fwd(p=p, zb=3) == EINVAL and fwd(p=p, M=-1) == EINVAL and fwd(p=p, C=-2) == EINVAL
        assert fwd(p=p, rm=b) == EINVAL and fwd(p=p, ws=None, rm=b, rv=b) == EINVAL and fwd(p=p, ws=None, nbt=b) == EINVAL
        assert fwd(p=p, mom=1.5) == EINVAL
        assert fwd(p=p, M=1) == EUNSUP
        assert fwd(p=p, z=odd) == EALIGN and fwd(p=p, ld=12) == EALIGN and fwd(p=p, ldyf=8) == EALIGN and fwd(p=p, ld=17) == EALIGN
        assert fwd(p=p, res=a, ldr=8) == EALIGN
        assert fwd(p=p, yb=c, ldyb=8, yf=None) == EALIGN
        assert fwd(p=p, M=0, z=None, g=None, yf=None) == 0 and fwd(p=p, C=0, z=None, mean=None) == 0
    assert fwd(p=1.0) == EINVAL and fwd(p=-0.5) == EINVAL and fwd(p=float("nan")) == EINVAL


def test_dr_backward_argument_errors(host):
    L, a, b, c, cell, odd = (host[k] for k in ("L", "a", "b", "c", "cell", "odd"))

    def bwd(second, z=a, zb=0, ld=16, g=a, ldg=16, gm=b, bt=b, mean=b, rstd=b, p=0.0, rng=cell, ws=c, dzb=None, lddzb=0, dzf=c,
            lddzf=16, M=4, C=16):
        if not second:
            return L.dhaug_bn_act_backward_partials_dr(z, zb, ld, g, ldg, gm, bt, mean, rstd, p, rng, 8, M, C, ws, None)
        return L.dhaug_bn_act_backward_dr(z, zb, ld, g, ldg, gm, bt, mean, rstd, p, rng, 8, ws, dzb, lddzb, dzf, lddzf, None, None, M,
                                          C, None)

    for second in (False, True):
        assert bwd(second, p=0.25, rng=None) == EINVAL
        assert bwd(second, p=0.25, rng=odd) == EALIGN
        assert bwd(second, p=0.0, rng=None, M=0, z=None, g=None, ws=None, dzf=None) == 0
        for p in (0.0, 0.25):
            assert bwd(second, p=p, z=None) == EINVAL and bwd(second, p=p, g=None) == EINVAL and bwd(second, p=p, rstd=None) == EINVAL
            assert bwd(second, p=p, ws=None) == EINVAL and bwd(second, p=p, zb=-1) == EINVAL and bwd(second, p=p, M=-1) == EINVAL
            assert bwd(second, p=p, ld=8) == EALIGN and bwd(second, p=p, g=odd) == EALIGN and bwd(second, p=p, ldg=18) == EALIGN
            assert bwd(second, p=p, M=0, z=None, g=None, ws=None, dzf=None) == 0
        assert bwd(second, p=1.0) == EINVAL
    for p in (0.0, 0.25):
        assert bwd(True, p=p, dzf=None) == EINVAL
        assert bwd(True, p=p, lddzf=8) == EALIGN and bwd(True, p=p, dzb=c, lddzb=8) == EALIGN


def test_u64_add_and_adam_lr_argument_errors(host):
    L, a, b, c, odd = (host[k] for k in ("L", "a", "b", "c", "odd"))
    assert L.dhaug_u64_add(None, 4, None) == EINVAL
    assert L.dhaug_u64_add(odd, 4, None) == EALIGN

    def adam(p=a, g=a, m=b, v=b, n=16, lr=c, step=c, max_norm=1.0, ws=c, norm=None):
        return L.dhaug_adam_clip_step_lr(p, g, m, v, n, lr, 0.9, 0.999, 1e-8, step, 1.0, max_norm, ws, norm, None)

    assert adam(lr=None) == EINVAL
    assert adam(lr=None, n=0) == EINVAL                       # (an empty vector does not excuse it)
    assert adam(lr=ctypes.c_void_p(c.value + 2)) == EALIGN
    # dhaug_adam_clip_step's own checks
    assert adam(n=-1) == EINVAL and adam(max_norm=0.0) == EINVAL and adam(max_norm=float("nan")) == EINVAL
    assert adam(step=None) == EINVAL and adam(ws=None) == EINVAL
    assert adam(p=None) == EINVAL and adam(g=None) == EINVAL and adam(m=None) == EINVAL and adam(v=None) == EINVAL
    assert adam(p=ctypes.c_void_p(a.value + 2)) == EALIGN and adam(ws=odd) == EALIGN
    assert adam(n=0, p=None, g=None, m=None, v=None) == 0


C_TYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "const uint64_t*": ctypes.c_void_p, "uint64_t*": ctypes.c_void_p, "uint16_t*": ctypes.c_void_p, "int64_t*": ctypes.c_void_p,
           "const int*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float}


def header_signature(hdr, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
    assert m, "%s is not declared in include/dhaug.h" % name
    out = []
    for arg in m.group(1).replace("\n", " ").split(","):
        ctype = arg.strip().rsplit(" ", 1)[0].strip()
        out.append(C_TYPES[ctype])
    return out


def test_ctypes_signatures_agree_with_the_header(built):
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    sig = built._lib.SIGNATURES
    for name in NEW:
        assert sig[name] == header_signature(hdr, name), name
    # the parser reads the entries they mirror the same way (it is not agreeing with itself only)
    for name in ("dhaug_bn_act_forward", "dhaug_bn_act_backward_partials", "dhaug_bn_act_backward", "dhaug_adam_clip_step"):
        assert sig[name] == header_signature(hdr, name), name
    # and a _dr entry differs from its twin in exactly the seed argument: a pointer to the cell in place of a 64-bit immediate
    for name in NEW[:3]:
        twin = sig[name[:-3]]
        diff = [i for i, (x, y) in enumerate(zip(sig[name], twin)) if x != y]
        assert len(sig[name]) == len(twin) and len(diff) == 1 and twin[diff[0]] == ctypes.c_uint64 and twin[diff[0] + 1] == ctypes.c_uint64
    lr, old = sig["dhaug_adam_clip_step_lr"], sig["dhaug_adam_clip_step"]
    assert [i for i, (x, y) in enumerate(zip(lr, old)) if x != y] == [5] and lr[5] == ctypes.c_void_p and old[5] == ctypes.c_float


def small_model(built):
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    cfg = NU.SMALL
    return TemporalModelOptimized1f(16, 2, 15, filter_widths=[1] * (cfg["stages"] + 1), dropout=0.25, channels=cfg["C"])


def test_graph_runner_on_cpu_raises_the_existing_error(built):
    from dhaug_amd.function_aug.model_pos_train import StepRunner
    m = small_model(built)
    opt = torch.optim.Adam(m.parameters())
    for graph in (False, True):
        with pytest.raises(RuntimeError, match="need a GPU"):
            StepRunner(m, opt, torch.nn.MSELoss(), torch.device("cpu"), graph=graph)


def test_graph_is_off_unless_asked_for(built, monkeypatch):
    from dhaug_amd.function_aug import model_pos_train as T
    monkeypatch.setattr(T, "POSENET_GRAPH", False)               # (DHAUG_POSENET_GRAPH as the module read it at import)
    assert T.graph_requested(argparse.Namespace()) is False
    assert T.graph_requested(argparse.Namespace(posenet_graph=False)) is False
    assert T.graph_requested(argparse.Namespace(posenet_graph=True)) is True
    monkeypatch.setattr(T, "POSENET_GRAPH", True)
    assert T.graph_requested(argparse.Namespace()) is True and T.graph_requested(argparse.Namespace(posenet_graph=False)) is True
    # the argument parser is as it was: the flag is an attribute a caller sets, not an option
    from dhaug_amd.function_aug.config import get_parse_args
    assert not hasattr(get_parse_args([]), "posenet_graph")


def test_device_dropout_stream_hands_out_the_eager_offsets(built, monkeypatch):
    """the host side of the stream: the k-th call of a step gets delta 4 k, the count runs on, advance() starts the next step at 0
    (its launch is replaced here: no GPU), and while the stream is set the torch generator is left alone"""
    from dhaug_amd import autograd_ops as A, ops
    added = []
    monkeypatch.setattr(ops, "u64_add", lambda cell, value: added.append(value))
    cell = torch.zeros(2, dtype=torch.int64)
    s = A.DeviceDropoutStream(cell)
    monkeypatch.setattr(A, "DEVICE_DROPOUT", s)
    got = [A.dropout_stream(torch.device("cpu")) for _ in range(3)]
    assert [d for _, d in got] == [0, 4, 8] and all(c is cell for c, _ in got)
    assert s.advance() == 3 and added == [12]
    assert A.dropout_stream(torch.device("cpu"))[1] == 0 and s.calls == 4
    assert s.advance() == 1 and s.advance() == 0 and added == [12, 4]
