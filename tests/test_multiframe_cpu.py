"""CPU-side checks of the multi-frame VideoPose posenets (models_Fk_GAN/mulit_farme_videopose.py): the state_dict interface against
the reference's recorded layout, the plain-torch path against records (a) and (a27) of tests/golden/posenet_multiframe.npz, the
dilated class against the strided class slid over the sequence, the construction errors, the new factory, and the argument errors
of the three tap entry points (before any launch)."""
import argparse
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import multiframe_util as MU
import posenet_util as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_ROUNDING = 2.0 ** -23


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def M(built):
    from dhaug_amd.models_Fk_GAN import mulit_farme_videopose
    return mulit_farme_videopose


@pytest.fixture(scope="module")
def G():
    return MU.load_golden()


@pytest.fixture(scope="module")
def fp32_gap():
    """the yardstick for fp32: how far the reference's single-frame class in fp32 lies from its own fp64 run, worst tensor of the
    records (a) of the two existing posenet fixtures, measured the way test_posenet_cpu.py does (and no less than one rounding)"""
    G64, G32 = NU.load_golden(), NU.load_golden(NU.GOLDEN_F32)
    worst = 0.0
    for rows in NU.ROWS_A:
        pre = "a%d_f64_" % rows
        for k in G64:
            if k.startswith(pre) and G64[k].dtype.kind == "f":
                ref, ref32 = np.asarray(G64[k], np.float64), np.asarray(G32["a%d_f32_%s" % (rows, k[len(pre):])], np.float64)
                worst = max(worst, float(np.abs(ref32 - ref).max() / np.abs(ref).max()))
    print("FIGURE reference fp32 against fp64 on the single-frame records (a), worst tensor %.3e" % worst)
    assert 0 < worst < 1e-5
    return max(worst, ONE_ROUNDING)


def make(M, cfg, strided=True, dropout=0.0, running=False):
    cls = M.multiFrame_TemporalModelOptimized1f if strided else M.multiFrame_TemporalModel
    m = cls(16, 2, 16, filter_widths=list(cfg["arch"]), dropout=dropout, channels=cfg["C"])
    m.load_state_dict(MU.seeded_state(cfg["C"], cfg["arch"], cfg["seed"], running=running), strict=True)
    return m


@pytest.mark.parametrize("arch", MU.LAYOUTS)
def test_state_dict_layout_is_the_references(M, G, arch):
    for cls in (M.multiFrame_TemporalModelOptimized1f, M.multiFrame_TemporalModel):
        m = cls(16, 2, 16, filter_widths=list(arch), causal=False, dropout=0.25, channels=1024)
        sd = m.state_dict()
        t = MU.tag(arch)
        assert list(sd.keys()) == [str(k) for k in G["keys_" + t]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in G["shapes_" + t]]
        assert [str(v.dtype) for v in sd.values()] == [str(s) for s in G["dtypes_" + t]]
        assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [(k, s, d) for k, (s, d) in MU.shapes(1024, arch).items()]
        assert m.receptive_field() == MU.receptive_field(arch) and m.total_causal_shift() == 0
        assert m.filter_widths == list(arch) and m.causal_shift == [0] * len(arch) and m.drop.p == 0.25
        assert m.pad == ([1, 3] if arch == (3, 3) else [1, 3, 9])
        m.set_bn_momentum(0.01)
        assert m.expand_bn.momentum == 0.01 and all(bn.momentum == 0.01 for bn in m.layers_bn)
        assert m.precision in ("bf16", "bf16x3", "bf16x6", "f16x3")


def test_one_seed_gives_the_stock_initial_weights(M):
    """the creation order is the reference's: torch's default initialisation draws the same numbers for a stock restatement"""
    for strided in (True, False):
        torch.manual_seed(7)
        ours = (M.multiFrame_TemporalModelOptimized1f if strided else M.multiFrame_TemporalModel)(16, 2, 16, [3, 3], channels=32)
        torch.manual_seed(7)
        stock = MU.StockMultiFrame(32, (3, 3), strided)
        for (k, a), (k2, b) in zip(ours.state_dict().items(), stock.state_dict().items()):
            assert k == k2 and torch.equal(a, b), k


@pytest.mark.parametrize("strided", [True, False])
def test_state_round_trips_through_stock_modules(M, strided):
    cfg = MU.SMALL
    m = make(M, cfg, strided, running=True)
    stock = MU.StockMultiFrame(cfg["C"], cfg["arch"], strided)
    stock.load_state_dict(m.state_dict(), strict=True)
    m2 = make(M, dict(cfg, seed=cfg["seed"] + 1), strided)
    m2.load_state_dict(stock.state_dict(), strict=True)
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    x = MU.dilated_input(cfg) if not strided else MU.record_inputs(cfg, 3)[0]
    m.eval(), stock.eval()
    with torch.no_grad():
        a, b = m(x), stock(x)
    assert a.shape == (x.shape[0], x.shape[1] - 8, 16, 3)
    assert (a - b).abs().max().item() <= 1e-5


def run_cpu(m, cfg, B, dtype):
    x, t = MU.record_inputs(cfg, B)
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


CASES = [("a%d_" % B, MU.SMALL, B) for B in MU.BATCH_A] + [("a27_%d_" % MU.BATCH_A27, MU.SMALL27, MU.BATCH_A27)]


@pytest.mark.parametrize("prefix,cfg,B", CASES, ids=[c[0] for c in CASES])
def test_cpu_path_matches_the_reference_record(M, G, fp32_gap, prefix, cfg, B):
    """records (a) and (a27): training output, loss, every gradient, the buffers, the evaluation output and the dilated class's
    output.  fp64: 1e-12 of each tensor's largest element.  fp32: 4 x fp32_gap."""
    names = [k[len(prefix):] for k in G if k.startswith(prefix)]
    blocks = len(cfg["arch"]) - 1
    assert len(names) == 4 + (3 + 2 * blocks + 2 * (1 + 2 * blocks)) + 3 * (1 + 2 * blocks)
    for dtype in (torch.float64, torch.float32):
        rec = run_cpu(make(M, cfg), cfg, B, dtype)
        dil = make(M, cfg, strided=False, running=True).to(dtype).eval()
        with torch.no_grad():
            rec["dil_out"] = dil(MU.dilated_input(cfg).to(dtype))
        assert set(rec) == set(names)
        bound = 1e-12 if dtype == torch.float64 else 4 * fp32_gap
        worst = 0.0
        for n in names:
            ref = torch.from_numpy(np.array(G[prefix + n]))
            if "num_batches" in n:
                assert int(rec[n]) == int(ref) == 1
                continue
            assert ref.dtype == torch.float64 and rec[n].shape == ref.shape, n
            err = (rec[n].double() - ref).abs().max().item() / ref.abs().max().item()
            worst = max(worst, err)
            assert err <= bound, (str(dtype), n, err, bound)
        print("FIGURE %s %s worst tensor %.3e (bound %.3e)" % (prefix, str(dtype), worst, bound))


@pytest.mark.parametrize("arch", [(3, 3), (3, 3, 3), (5, 3), (3,), (1, 3)])
def test_dilated_equals_the_strided_model_slid_over_the_sequence(M, arch):
    cfg = dict(C=32, arch=arch, seed=31)
    s = make(M, cfg, True, running=True).double().eval()
    d = make(M, cfg, False, running=True).double().eval()
    rf = MU.receptive_field(arch)
    assert s.receptive_field() == d.receptive_field() == rf
    x = MU.make_inputs(2, rf + 6, 9)[0].double()
    with torch.no_grad():
        yd, ys = d(x), MU.slide(s, x)
    assert yd.shape == ys.shape == (2, 7, 16, 3)
    assert (yd - ys).abs().max().item() <= 1e-12 * ys.abs().max().item()


def test_construction_errors(M):
    S, D = M.multiFrame_TemporalModelOptimized1f, M.multiFrame_TemporalModel
    for cls in (S, D):
        with pytest.raises(NotImplementedError, match="causal"):
            cls(16, 2, 16, [3, 3], causal=True, channels=64)
        with pytest.raises(ValueError, match="odd filter widths"):
            cls(16, 2, 16, [3, 2], channels=64)
        with pytest.raises(ValueError, match="multiple of 16"):
            cls(16, 2, 16, [3, 3], channels=40)
    with pytest.raises(NotImplementedError, match="dense"):
        D(16, 2, 16, [3, 3], channels=64, dense=True)
    with pytest.raises(TypeError):
        S(16, 2, 16, [3, 3], channels=64, dense=True)
    m = S(16, 2, 16, [3, 3], channels=64)
    with pytest.raises(ValueError, match="input must be"):
        m(torch.zeros(4, 9, 17, 2))
    with pytest.raises(ValueError, match="receptive field"):
        m(torch.zeros(4, 5, 16, 2))


def test_multi_frame_model_pos_preparation(built, M, tmp_path, capsys):
    from dhaug_amd.function_baseline.model_pos_preparation import model_pos_preparation, multi_frame_model_pos_preparation
    args = argparse.Namespace(posenet_name="mulit_farme_videopose", architecture="3,3", pretrain=False, stages=2)
    cpu = torch.device("cpu")
    train = multi_frame_model_pos_preparation(args, None, cpu)
    assert type(train) is M.multiFrame_TemporalModelOptimized1f and train.filter_widths == [3, 3] and train.channels == 1024
    assert train.drop.p == 0.25 and train.shrink.weight.shape == (48, 1024, 1) and train.expand_conv.weight.shape == (1024, 32, 3)
    args.architecture = "3,3,3"
    test = multi_frame_model_pos_preparation(args, None, cpu, flag="test")
    assert type(test) is M.multiFrame_TemporalModel and test.receptive_field() == 27 and len(test.layers_conv) == 4
    # a checkpoint saved from the other class
    path = str(tmp_path / "ckpt.pth.tar")
    torch.save({"model_pos": test.state_dict()}, path)
    args.pretrain, args.posenet_pretrain_path = True, path
    loaded = multi_frame_model_pos_preparation(args, None, cpu, flag="train")
    assert type(loaded) is M.multiFrame_TemporalModelOptimized1f
    assert all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), test.state_dict().values()))
    args.posenet_pretrain_path = None
    with pytest.raises(ValueError, match="posenet_pretrain_path"):
        multi_frame_model_pos_preparation(args, None, cpu)
    args.pretrain = False
    with pytest.raises(ValueError, match="flag"):
        multi_frame_model_pos_preparation(args, None, cpu, flag="valid")
    for name in ("gcn", "mlp", "videopose", "mulit_farme_poseformer", "nonsense"):
        args.posenet_name = name
        with pytest.raises(NotImplementedError, match="mulit_farme_videopose"):
            multi_frame_model_pos_preparation(args, None, cpu)
    # the old factory still refuses the name
    args.posenet_name = "mulit_farme_videopose"
    with pytest.raises(NotImplementedError, match="videopose"):
        model_pos_preparation(args, None, cpu)


def test_f16x3_runs_as_bf16x6(M):
    m = make(M, MU.SMALL)
    m.precision = "f16x3"
    assert m._arithmetic() == "bf16x6"
    m.precision = "bf16x3"
    assert m._arithmetic() == "bf16x3"


def test_tap_entry_points_argument_errors(built):
    """csrc/dhaug_taps.hip: a bad argument comes back as the documented code before any launch -- every pointer here is a valid HOST
    address, so a call that got as far as a launch would return a HIP error -- and an empty problem looks at no pointer"""
    L = built._lib.lib()
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c = ctypes.c_void_p(base), ctypes.c_void_p(base + 8192), ctypes.c_void_p(base + 16384)
    odd = ctypes.c_void_p(base + 4)
    EINVAL, EALIGN, EUNSUP = -1, -2, -3

    def pack(W=a, N=4, Cin=16, k=3, nt=b, ld_nt=48, nn=c, ld_nn=16):
        return L.dhaug_conv_taps_pack_bf16(W, N, Cin, k, nt, ld_nt, nn, ld_nn, None)

    assert pack(N=-1) == EINVAL and pack(Cin=-16) == EINVAL and pack(W=None) == EINVAL and pack(nt=None) == EINVAL
    assert pack(ld_nt=40) == EINVAL and pack(ld_nn=8) == EINVAL
    assert pack(k=0) == EUNSUP and pack(k=17) == EUNSUP and pack(Cin=24) == EUNSUP and pack(Cin=8) == EUNSUP
    assert pack(N=1 << 30, Cin=16, k=16) == EUNSUP
    assert pack(W=odd) == EALIGN and pack(nt=odd) == EALIGN and pack(nn=odd) == EALIGN and pack(ld_nt=52) == EALIGN
    assert pack(ld_nn=20) == EALIGN
    assert pack(N=0, W=None, nt=None, nn=None) == 0 and pack(Cin=0, W=None, nt=None, nn=None) == 0

    def perm(src=a, dst=b, N=4, Cin=5, k=3, to_taps=1, acc=0):
        return L.dhaug_conv_taps_permute_f32(src, dst, N, Cin, k, to_taps, acc, None)

    assert perm(N=-1) == EINVAL and perm(k=-1) == EINVAL and perm(to_taps=2) == EINVAL and perm(acc=2) == EINVAL
    assert perm(to_taps=1, acc=1) == EINVAL and perm(src=None) == EINVAL and perm(dst=None) == EINVAL and perm(dst=a) == EINVAL
    assert perm(N=1 << 20, Cin=1 << 10, k=2) == EUNSUP
    assert perm(dst=odd) == EALIGN and perm(src=ctypes.c_void_p(base + 2)) == EALIGN
    assert perm(N=0, src=None, dst=None) == 0 and perm(k=0, src=None, dst=None) == 0 and perm(Cin=0, src=None, dst=None) == 0

    def gather(x=a, xb=0, ld_x=16, nseq=2, t_in=5, C=16, k=3, dil=1, stride=1, ob=b, ld_ob=48, of=c, ld_of=48):
        return L.dhaug_tap_gather(x, xb, ld_x, nseq, t_in, C, k, dil, stride, ob, ld_ob, of, ld_of, None)

    assert gather(nseq=-1) == EINVAL and gather(t_in=-1) == EINVAL and gather(C=-16) == EINVAL and gather(xb=2) == EINVAL
    assert gather(dil=0) == EINVAL and gather(stride=0) == EINVAL and gather(x=None) == EINVAL and gather(ob=None, of=None) == EINVAL
    assert gather(xb=1) == EINVAL                                  # fp32 output needs fp32 input
    assert gather(ld_x=8) == EINVAL and gather(ld_ob=40) == EINVAL and gather(ld_of=44) == EINVAL
    assert gather(C=24) == EUNSUP and gather(k=0) == EUNSUP and gather(k=17) == EUNSUP
    assert gather(t_in=2) == EUNSUP and gather(dil=3, t_in=6) == EUNSUP and gather(t_in=0) == EUNSUP          # t_out < 1
    assert gather(nseq=1 << 20, t_in=1 << 11) == EUNSUP and gather(dil=1 << 30) == EUNSUP
    assert gather(x=odd) == EALIGN and gather(ob=odd) == EALIGN and gather(of=odd) == EALIGN
    assert gather(ld_x=18) == EALIGN and gather(ld_ob=52) == EALIGN and gather(ld_of=50) == EALIGN
    assert gather(xb=1, of=None, ld_x=20) == EALIGN
    assert gather(nseq=0, x=None, ob=None, of=None) == 0 and gather(C=0, x=None, ob=None, of=None) == 0


def test_launch_constants_mirror_the_sources():
    """tests/multiframe_util's launch constants are the kernels' (the sizes of the GPU kernel tests are derived from them)"""
    src = open(MU.TAPS_SOURCE).read()
    common = open(os.path.join(os.path.dirname(MU.TAPS_SOURCE), "dhaug_common.h")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert const("kBlock") == MU.BLOCK and const("kTileN") == MU.TILE_N and const("kTileC") == MU.TILE_C
    assert const("kPermuteVec") == MU.PERMUTE_VEC and const("kGatherRows") == MU.GATHER_ROWS and const("kMaxTaps") == MU.MAX_TAPS
    assert re.search(r"int max_blocks = 256 \* 8\)", common) and MU.MAX_BLOCKS == 256 * 8
    assert MU.PERMUTE_SPAN == MU.BLOCK * MU.PERMUTE_VEC
