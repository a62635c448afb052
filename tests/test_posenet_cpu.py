"""CPU-side checks of the single-frame VideoPose posenet: the state_dict interface against the reference's recorded layout, the
factory, the plain-torch path against record (a) of tests/golden/posenet_videopose.npz, and the argument errors of the BatchNorm
entry points (before any launch)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import posenet_util as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def G():
    return NU.load_golden()


@pytest.fixture(scope="module")
def G32():
    return NU.load_golden(NU.GOLDEN_F32)


# the least fp32 bound of a tensor: one rounding of its largest element.  The reference's fp32 run can land closer to its fp64 run
# than that by luck (a loss that rounds to the same float), which another fp32 evaluation order cannot be asked to repeat.
ONE_ROUNDING = 2.0 ** -23


def make(built, cfg, dropout=0.0):
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    m = TemporalModelOptimized1f(16, 2, 15, filter_widths=[1] * (cfg["stages"] + 1), dropout=dropout, channels=cfg["C"])
    m.load_state_dict(NU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"]), strict=True)
    return m


def test_state_dict_layout_is_the_references(built, G):
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    m = TemporalModelOptimized1f(16, 2, 15, filter_widths=[1] * 5, causal=False, dropout=0.25, channels=1024)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in G["keys_1024_4"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in G["shapes_1024_4"]]
    assert [str(v.dtype) for v in sd.values()] == [str(s) for s in G["dtypes_1024_4"]]
    assert sum(p.numel() for p in m.parameters()) == 8485933
    # the test utilities' layout is the same one
    assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [(k, s, d) for k, (s, d) in NU.shapes(1024, 4).items()]
    assert m.receptive_field() == 1
    m.set_bn_momentum(0.01)
    assert m.expand_bn.momentum == 0.01 and all(bn.momentum == 0.01 for bn in m.layers_bn)
    assert m.precision in ("bf16", "bf16x3", "bf16x6", "f16x3")


def test_single_frame_is_the_strided_model_at_k1(built):
    """the single-frame class and the strided multi-frame class with every filter width 1, built under one seed: the same keys in
    the same order, the same shapes and the same initial values (one constructor, one order of creation and of random draws)"""
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    from dhaug_amd.models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModelOptimized1f
    states = []
    for cls in (TemporalModelOptimized1f, multiFrame_TemporalModelOptimized1f):
        torch.manual_seed(3)
        states.append(cls(16, 2, 15, [1] * 3, channels=64).state_dict())
    assert list(states[0].keys()) == list(states[1].keys()) == list(NU.shapes(64, 2).keys())
    for k, a in states[0].items():
        b = states[1][k]
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), k


def test_state_round_trips_through_stock_modules(built):
    cfg = NU.SMALL
    m = make(built, cfg)
    stock = NU.StockPosenet(cfg["C"], cfg["stages"])
    stock.load_state_dict(m.state_dict(), strict=True)
    m2 = make(built, dict(cfg, seed=cfg["seed"] + 1))
    m2.load_state_dict(stock.state_dict(), strict=True)
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    x, _ = NU.make_inputs(7, 5)
    m.eval(), stock.eval()
    with torch.no_grad():
        a, b = m(x), stock(x)
    assert a.shape == (7, 16, 3) and torch.all(a[:, 0] == 0)
    assert (a - b).abs().max().item() <= 1e-5
    assert torch.equal(m(x.reshape(7, 32)), m(x))


def test_model_pos_preparation(built, capsys):
    from dhaug_amd.function_baseline.model_pos_preparation import model_pos_preparation
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    args = argparse.Namespace(posenet_name="videopose", stages=2, pretrain=False, dropout=0.25)
    m = model_pos_preparation(args, None, torch.device("cpu"))
    assert isinstance(m, TemporalModelOptimized1f) and len(m.layers_conv) == 4 and m.channels == 1024 and m.drop.p == 0.25
    args.stages = 4
    assert len(model_pos_preparation(args, None, torch.device("cpu"), flag="test").layers_conv) == 8
    for name in ("gcn", "mlp", "mulit_farme_videopose", "mulit_farme_poseformer", "nonsense"):
        args.posenet_name = name
        with pytest.raises(NotImplementedError, match="videopose"):
            model_pos_preparation(args, None, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="filter width"):
        TemporalModelOptimized1f(16, 2, 15, filter_widths=[1, 3], channels=64)
    with pytest.raises(NotImplementedError, match="causal"):
        TemporalModelOptimized1f(16, 2, 15, filter_widths=[1, 1], causal=True, channels=64)


def test_pretrained_checkpoint_loads(built, tmp_path):
    from dhaug_amd.function_baseline.model_pos_preparation import model_pos_preparation
    state = NU.seeded_state(1024, 1, 3)
    path = str(tmp_path / "ckpt.pth.tar")
    torch.save({"model_pos": state}, path)
    args = argparse.Namespace(posenet_name="videopose", stages=1, pretrain=True, posenet_pretrain_path=path)
    m = model_pos_preparation(args, None, torch.device("cpu"))
    assert all(torch.equal(a, state[k]) for k, a in m.state_dict().items())
    args.posenet_pretrain_path = None
    with pytest.raises(ValueError, match="posenet_pretrain_path"):
        model_pos_preparation(args, None, torch.device("cpu"))


def run_cpu(m, M, cfg, dtype):
    x, t = NU.make_inputs(M, cfg["seed"] + 100 + M)
    m = m.to(dtype).train()
    out = m(x.to(dtype))
    loss = torch.nn.functional.mse_loss(out, t.to(dtype))
    loss.backward()
    rec = dict(out=out.detach(), loss=loss.detach().reshape(1))
    rec.update({"grad_" + k: p.grad for k, p in m.named_parameters()})
    rec.update({"buf_" + k: b.detach().clone() for k, b in m.named_buffers()})
    m.eval()
    with torch.no_grad():
        rec["eval_out"] = m(x.to(dtype))
    return rec


@pytest.mark.parametrize("M", NU.ROWS_A)
def test_cpu_path_matches_the_reference_record(built, G, G32, M):
    """record (a): training output, loss, every gradient, the buffers and the evaluation output.  fp64: 1e-12 of each tensor's
    largest element.  fp32: per tensor, 4 x the distance of the reference class's own fp32 run from its fp64 run, computed here
    from the two records (and no less than 4 x ONE_ROUNDING)."""
    cfg = NU.SMALL
    names = [k[len("a%d_f64_" % M):] for k in G if k.startswith("a%d_f64_" % M)]
    assert len(names) == 3 + 17 + 15
    runs = {torch.float64: run_cpu(make(built, cfg), M, cfg, torch.float64), torch.float32: run_cpu(make(built, cfg), M, cfg, torch.float32)}
    for dtype, rec in runs.items():
        assert set(rec) == set(names)
        for n in names:
            ref = torch.from_numpy(np.array(G["a%d_f64_%s" % (M, n)]))
            ref32 = torch.from_numpy(np.array(G32["a%d_f32_%s" % (M, n)]))
            if "num_batches" in n:
                assert int(rec[n]) == int(ref) == int(ref32) == 1
                continue
            assert ref32.dtype == torch.float32 and ref.dtype == torch.float64
            scale = ref.abs().max().item()
            own = (ref32.double() - ref).abs().max().item() / scale
            bound = 1e-12 if dtype == torch.float64 else 4 * max(own, ONE_ROUNDING)
            err = (rec[n].double() - ref).abs().max().item() / scale
            print("FIGURE a%d %s %s err %.3e reference fp32 %.3e" % (M, str(dtype), n, err, own))
            assert err <= bound, (str(dtype), n, err, bound)


def test_wide_fp32_record_documents_the_reference(G, G32):
    """record (b): the reference's fp32 run against its fp64 run on the recorded samples (the figure the fixture's generator
    explains: fp64 is the yardstick), and the two records cover the same tensors"""
    names = sorted(k[len("b_f64_"):] for k in G if k.startswith("b_f64_"))
    assert names == sorted(k[len("b_f32_"):] for k in G32 if k.startswith("b_f32_")) and len(names) > 60
    worst = 0.0
    for n in names:
        if n.endswith("__full") or n.endswith("__sample"):
            a, b = np.asarray(G["b_f64_" + n], np.float64), np.asarray(G32["b_f32_" + n], np.float64)
            worst = max(worst, float(np.abs(a - b).max() / np.abs(a).max()))
    print("FIGURE b reference fp32 against fp64, worst tensor %.3e" % worst)
    assert 0 < worst < 1e-5


def test_restatement_matches_the_reference_record(G):
    """tests/posenet_util.network_ref (the GPU kernel tests' yardstick) against record (a)"""
    cfg = NU.SMALL
    for M in NU.ROWS_A:
        x, t = NU.make_inputs(M, cfg["seed"] + 100 + M)
        r = NU.network_ref(NU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"]), x, t)
        pairs = [("out", r["out"]), ("loss", r["loss"].reshape(1)), ("eval_out", r["eval_out"])]
        pairs += [("grad_" + k, v) for k, v in r["grads"].items()] + [("buf_" + k, v) for k, v in r["buffers"].items()]
        assert len(pairs) == 3 + 17 + 10
        for n, v in pairs:
            ref = torch.from_numpy(np.array(G["a%d_f64_%s" % (M, n)]))
            assert (v - ref).abs().max().item() <= 1e-12 * ref.abs().max().item(), n


def test_posenet_adam_layout_and_checkpoint(built):
    """PosenetAdam places the 45-element output bias (180 bytes) behind the other tensors, so every tensor in front of it starts on
    the 16-byte grid of the flat buffer; its state_dict carries the layout and moments saved under another layout are refused"""
    from dhaug_amd.optim import PosenetAdam
    m = make(built, NU.SMALL)
    given = list(m.parameters())
    opt = PosenetAdam(given, lr=1e-3)
    assert opt._params[-1] is m.shrink.bias and opt._reordered
    assert [p for p in opt._params[:-1]] == [p for p in given if p is not m.shrink.bias]          # a stable sort
    base = opt.flat_param.data_ptr()
    assert all((p.data_ptr() - base) % 16 == 0 for p in opt._params)
    sd = opt.state_dict()
    assert sd["dhaug_flat"]["layout"] == [p.numel() for p in opt._params]
    opt.load_state_dict(sd)
    old = {k: (dict(v) if k == "dhaug_flat" else v) for k, v in sd.items()}
    del old["dhaug_flat"]["layout"]
    with pytest.raises(RuntimeError, match="layout"):
        opt.load_state_dict(old)
    old["dhaug_flat"]["layout"] = [p.numel() for p in given]
    with pytest.raises(RuntimeError, match="layout"):
        opt.load_state_dict(old)
    # a model the rule leaves alone loads a checkpoint without a layout as before
    lin = torch.nn.Linear(8, 45)
    o2 = PosenetAdam(lin.parameters())
    s2 = o2.state_dict()
    del s2["dhaug_flat"]["layout"]
    assert not o2._reordered
    o2.load_state_dict(s2)


def test_f16x3_runs_as_bf16x6(built):
    m = make(built, NU.SMALL)
    m.precision = "f16x3"
    assert m._arithmetic() == "bf16x6"
    m.precision = "bf16x3"
    assert m._arithmetic() == "bf16x3"


def test_one_row_in_training_raises(built):
    m = make(built, NU.SMALL).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 16, 2))
    m.eval()
    with torch.no_grad():
        assert m(torch.zeros(1, 16, 2)).shape == (1, 16, 3)
    with pytest.raises(ValueError, match="input must be"):
        m(torch.zeros(4, 17, 2))


def test_batchnorm_argument_errors(built):
    """the BatchNorm entry points (csrc/dhaug_posenet.hip): a bad argument comes back as the documented code before any launch --
    every pointer here is a valid HOST address, so a call that got as far as a launch would return a HIP error -- and an empty
    batch is a no-op that looks at no pointer"""
    L = built._lib.lib()
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c = ctypes.c_void_p(base), ctypes.c_void_p(base + 8192), ctypes.c_void_p(base + 16384)
    odd = ctypes.c_void_p(base + 4)
    EINVAL, EALIGN, EUNSUP = -1, -2, -3
    # partials: z_bf16 in {0, 1}, sizes >= 0, z / workspace not null, rows 16-byte aligned, ld >= C
    assert L.dhaug_bn_partials(a, 2, 16, 4, 16, b, None) == EINVAL
    assert L.dhaug_bn_partials(a, 0, 16, -1, 16, b, None) == EINVAL
    assert L.dhaug_bn_partials(None, 0, 16, 4, 16, b, None) == EINVAL
    assert L.dhaug_bn_partials(a, 0, 16, 4, 16, None, None) == EINVAL
    assert L.dhaug_bn_partials(odd, 0, 16, 4, 16, b, None) == EALIGN
    assert L.dhaug_bn_partials(a, 0, 12, 4, 16, b, None) == EALIGN            # short leading dimension
    assert L.dhaug_bn_partials(a, 0, 18, 4, 16, b, None) == EALIGN            # rows off the 16-byte grid
    assert L.dhaug_bn_partials(a, 1, 20, 4, 16, b, None) == EALIGN
    assert L.dhaug_bn_partials(a, 0, 1 << 31, 4, 1 << 30, b, None) == EUNSUP
    assert L.dhaug_bn_partials(None, 0, 0, 0, 16, None, None) == 0
    assert L.dhaug_bn_partials(None, 1, 0, 4, 0, None, None) == 0

    def fwd(z=a, zb=0, ld=16, res=None, ldr=0, g=b, bt=b, mean=b, rstd=b, ws=c, rm=None, rv=None, nbt=None, mom=0.1, eps=1e-5,
            p=0.0, yb=None, ldyb=0, yf=c, ldyf=16, M=4, C=16):
        return L.dhaug_bn_act_forward(z, zb, ld, res, ldr, g, bt, mean, rstd, ws, rm, rv, nbt, mom, eps, p, 1, 0, yb, ldyb, yf, ldyf,
                                      M, C, None)

    assert fwd(z=None) == EINVAL and fwd(g=None) == EINVAL and fwd(mean=None) == EINVAL and fwd(yf=None) == EINVAL
    assert fwd(zb=3) == EINVAL and fwd(M=-1) == EINVAL and fwd(C=-2) == EINVAL
    assert fwd(p=1.0) == EINVAL and fwd(p=-0.5) == EINVAL and fwd(p=float("nan")) == EINVAL
    assert fwd(rm=b) == EINVAL                                    # the running buffers come together
    assert fwd(ws=None, rm=b, rv=b) == EINVAL                     # given statistics update nothing
    assert fwd(ws=None, nbt=b) == EINVAL
    assert fwd(mom=1.5) == EINVAL
    assert fwd(M=1) == EUNSUP                                     # batch statistics of one row
    assert fwd(z=odd) == EALIGN and fwd(ld=12) == EALIGN and fwd(ldyf=8) == EALIGN and fwd(ld=17) == EALIGN
    assert fwd(res=a, ldr=8) == EALIGN
    assert fwd(yb=c, ldyb=8, yf=None) == EALIGN                   # bf16 rows shorter than ceil16(C)
    assert fwd(yb=c, ldyb=40, yf=None, C=40, ld=40) == EALIGN     # C = 40 pads to 48
    assert fwd(M=0, z=None, g=None, yf=None) == 0 and fwd(C=0, z=None, mean=None) == 0

    def bwd(second, z=a, zb=0, ld=16, g=a, ldg=16, gm=b, bt=b, mean=b, rstd=b, p=0.0, ws=c, dzb=None, lddzb=0, dzf=c, lddzf=16,
            M=4, C=16):
        if not second:
            return L.dhaug_bn_act_backward_partials(z, zb, ld, g, ldg, gm, bt, mean, rstd, p, 1, 0, M, C, ws, None)
        return L.dhaug_bn_act_backward(z, zb, ld, g, ldg, gm, bt, mean, rstd, p, 1, 0, ws, dzb, lddzb, dzf, lddzf, None, None, M, C,
                                       None)

    for second in (False, True):
        assert bwd(second, z=None) == EINVAL and bwd(second, g=None) == EINVAL and bwd(second, rstd=None) == EINVAL
        assert bwd(second, ws=None) == EINVAL and bwd(second, zb=-1) == EINVAL and bwd(second, p=1.0) == EINVAL
        assert bwd(second, M=-1) == EINVAL
        assert bwd(second, ld=8) == EALIGN and bwd(second, g=odd) == EALIGN and bwd(second, ldg=18) == EALIGN
        assert bwd(second, M=0, z=None, g=None, ws=None, dzf=None) == 0
    assert bwd(True, dzf=None) == EINVAL
    assert bwd(True, lddzf=8) == EALIGN and bwd(True, dzb=c, lddzb=8) == EALIGN

    def fold(W=a, ldw=8, g=b, bt=b, rm=b, rv=b, eps=1e-5, Wo=c, ldo=8, bo=c, ro=c, N=4, K=8):
        return L.dhaug_bn_fold(W, ldw, g, bt, rm, rv, eps, Wo, ldo, bo, ro, N, K, None)

    assert fold(g=None) == EINVAL and fold(rv=None) == EINVAL and fold(W=None) == EINVAL and fold(N=-1) == EINVAL
    assert fold(Wo=None, bo=None, ro=None) == EINVAL and fold(eps=-1.0) == EINVAL
    assert fold(ldw=4) == EALIGN and fold(ldo=4) == EALIGN and fold(g=ctypes.c_void_p(base + 2)) == EALIGN
    assert fold(N=1 << 30) == EUNSUP
    assert fold(N=0, g=None, W=None, Wo=None, bo=None, ro=None) == 0


def test_launch_constants_mirror_the_sources(built):
    """tests/posenet_util's launch constants are the kernels' (the multi-pass sizes of the GPU tests are derived from them)"""
    import re
    src = open(os.path.join(ROOT, "dh-aug-dh-forward-kinematics-model-driven-augmentation-for-3d-human-pose-estimation_amd", "csrc",
                            "dhaug_posenet.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    assert int(re.search(r"constexpr int kLanesPerRow = (\d+);", src).group(1)) == NU.LANES_PER_ROW
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == NU.LANES_PER_ROW * NU.ROWS_PER_PASS
    assert int(re.search(r"#define\s+DHAUG_BN_MAX_CHUNKS\s+(\d+)", hdr).group(1)) == NU.MAX_CHUNKS == built._lib.BN_MAX_CHUNKS
    M, C = NU.MULTIPASS
    strips, chunks, rpc = NU.launch_of(M, C, torch.float32)
    assert chunks > 1 and rpc >= 2 * NU.ROWS_PER_PASS and strips == 2
    assert NU.launch_of(1024, 1024, torch.float32)[:2] == (32, 8) and NU.launch_of(1024, 1024, torch.bfloat16)[:2] == (16, 16)
