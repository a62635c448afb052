"""CPU-side checks of the SemGCN posenet: the state_dict interface against the reference's recorded layout and initialisation, the
factory, the plain-torch path and the tests' own restatement against record (a) of tests/golden/posenet_gcn.npz, and the
argument errors of the graph entry points (before any launch)."""
import argparse
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import gcn_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dh-aug-dh-forward-kinematics-model-driven-augmentation-for-3d-human-pose-estimation_amd")

# the least fp32 bound of a tensor: one rounding of its largest element (the rule of test_posenet_cpu.py)
ONE_ROUNDING = 2.0 ** -23


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def G():
    return CU.load_golden()


@pytest.fixture(scope="module")
def G32():
    return CU.load_golden(CU.GOLDEN_F32)


def make(built, cfg, dropout=None, load=True):
    from dhaug_amd.models_baseline.gcn import SemGCN
    m = SemGCN(CU.adj_matrix(), cfg["hid"], num_layers=cfg["blocks"], p_dropout=dropout)
    if load:
        m.load_state_dict(CU.seeded_state(cfg["hid"], cfg["blocks"], cfg["seed"]), strict=True)
    return m


def test_state_dict_layout_is_the_references(built, G):
    from dhaug_amd.models_baseline.gcn import H36M_PARENTS, SemGCN, adj_mx_from_parents
    assert list(H36M_PARENTS) == [int(p) for p in G["parents"]] == CU.PARENTS
    adj = adj_mx_from_parents(H36M_PARENTS)
    assert adj.dtype == torch.float32 and torch.equal(adj, CU.adj_matrix())
    assert np.array_equal((adj > 0).numpy(), G["adj_mask"]) and int((adj > 0).sum()) == 46 and int((adj > 0).sum(1).max()) == 5
    m = SemGCN(adj, 128, num_layers=4, p_dropout=0.25)
    sd = m.state_dict()
    assert len(sd) == 75 == len(G["keys_128_4"])
    assert list(sd.keys()) == [str(k) for k in G["keys_128_4"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in G["shapes_128_4"]]
    assert [str(v.dtype) for v in sd.values()] == [str(s) for s in G["dtypes_128_4"]]
    assert sum(p.numel() for p in m.parameters()) == 267343 == int(G["param_count"])
    assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [(k, s, d) for k, (s, d) in CU.shapes(128, 4).items()]
    # e follows the row-major order of the pattern: [0,0], [0,1], [0,4], [0,7], [1,0], [1,1], ...
    g = m.gconv_output
    assert list(zip(g.rows, g.cols))[:6] == [(0, 0), (0, 1), (0, 4), (0, 7), (1, 0), (1, 1)]
    assert (g.rows, g.cols) == CU.pattern()
    assert "adj" not in sd and m.precision in ("bf16", "bf16x3", "bf16x6", "f16x3")
    assert m.gconv_input[0].dropout.p == 0.25 and m.gconv_layers[3].gconv2.dropout.p == 0.25


def test_seeded_construction_is_the_references(built, G):
    """one seed gives the stock container's initial state tensor for tensor -- the same order of parameter creation and random
    draws -- and both give the state the reference's own constructor was recorded with"""
    from dhaug_amd.models_baseline.gcn import SemGCN
    cfg = CU.INIT
    torch.manual_seed(cfg["seed"])
    ours = SemGCN(CU.adj_matrix(), cfg["hid"], num_layers=cfg["blocks"], p_dropout=0.25).state_dict()
    torch.manual_seed(cfg["seed"])
    stock = CU.StockGCN(cfg["hid"], cfg["blocks"], 0.25).state_dict()
    assert list(ours) == list(stock) and len(ours) == 3 * 8 + 3
    for k in ours:
        assert torch.equal(ours[k], stock[k]), k
        assert torch.equal(ours[k], torch.from_numpy(np.array(G["init_" + k]))), k
    assert torch.all(ours["gconv_output.e"] == 1) and ours["gconv_output.W"].abs().max() > 0


def test_state_round_trips_through_the_stock_container(built):
    cfg = CU.SMALL
    m = make(built, cfg)
    stock = CU.StockGCN(cfg["hid"], cfg["blocks"])
    stock.load_state_dict(m.state_dict(), strict=True)
    m2 = make(built, dict(cfg, seed=cfg["seed"] + 1))
    m2.load_state_dict(stock.state_dict(), strict=True)
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    x, _ = CU.make_inputs(7, 5)
    m.eval(), stock.eval()
    with torch.no_grad():
        a, b = m(x), stock(x)
    assert a.shape == (7, 16, 3)
    assert (a - b).abs().max().item() <= 1e-5
    assert torch.equal(m(x.reshape(7, 32)), m(x))
    with pytest.raises(ValueError, match="input must be"):
        m(torch.zeros(4, 17, 2))


def check_record_a(rec, G, G32, B, dtype, what):
    """fp64: 1e-12 of each tensor's yardstick.  fp32: per tensor, 4 x the distance of the reference class's own fp32 run from its
    fp64 run, computed here from the two records (and no less than 4 x ONE_ROUNDING)."""
    prefix = "a%d_f64_" % B
    names = [k[len(prefix):] for k in G if k.startswith(prefix)]
    assert [n for n, _ in rec] == names and len(names) == 3 + 5 * 5 + 3 + 5 * 3
    ref32 = [(n, torch.from_numpy(np.array(G32["a%d_f32_%s" % (B, n)]))) for n in names]
    own = CU.errors_whole(ref32, G, prefix)
    err = CU.errors_whole(rec, G, prefix)
    assert len(err) == 3 + 5 * 5 + 3 + 5 * 2
    for n, e in err.items():
        bound = 1e-12 if dtype == torch.float64 else 4 * max(own[n], ONE_ROUNDING)
        print("FIGURE a%d %s %s %s err %.3e reference fp32 %.3e" % (B, what, str(dtype), n, e, own[n]))
        assert e <= bound, (what, str(dtype), n, e, bound)


@pytest.mark.parametrize("B", CU.ROWS_A)
def test_restatement_matches_the_reference_record(G, G32, B):
    """tests/gcn_util.network_ref (the GPU tests' yardstick and stock side) against record (a)"""
    cfg = CU.SMALL
    x, t = CU.inputs_of(cfg, B)
    state = CU.seeded_state(cfg["hid"], cfg["blocks"], cfg["seed"])
    check_record_a(CU.network_ref(state, x, t), G, G32, B, torch.float64, "restatement")


@pytest.mark.parametrize("B", CU.ROWS_A)
def test_cpu_path_matches_the_reference_record(built, G, G32, B):
    """record (a): training output, loss, every gradient (e included), the buffers and the evaluation output"""
    cfg = CU.SMALL
    x, t = CU.inputs_of(cfg, B)
    for dtype in (torch.float64, torch.float32):
        m = make(built, cfg).to(dtype)
        check_record_a(CU.run_record(m, x.to(dtype), t.to(dtype)), G, G32, B, dtype, "module")


def test_wide_fp32_record_documents_the_reference(G, G32):
    """record (b): the two records cover the same tensors, and the reference's fp32 run lies within 1e-5 of its fp64 run on them"""
    names = sorted(k[len("b_f64_"):] for k in G if k.startswith("b_f64_"))
    assert names == sorted(k[len("b_f32_"):] for k in G32 if k.startswith("b_f32_")) and len(names) > 70
    tensors = sorted({n.rsplit("__", 1)[0] for n in names if "__" in n})
    rec = []
    for i, n in enumerate(tensors):
        part = CU.compact_ref(G32, "b_f32_", n)
        rec.append((n, part["full" if "full" in part else "sample"]))
    worst = 0.0
    for n, v in rec:
        ref = CU.compact_ref(G, "b_f64_", n)
        sref = CU.compact_ref(G, "b_f64_", CU.scale_name(n, set(tensors)))
        scale = sref["full" if "full" in sref else "sample"].double().abs().max().item()
        worst = max(worst, (v.double() - ref["full" if "full" in ref else "sample"].double()).abs().max().item() / scale)
    print("FIGURE b reference fp32 against fp64, worst tensor %.3e" % worst)
    assert 0 < worst < 1e-5


class _Skeleton:
    def __init__(self, parents):
        self._p = list(parents)

    def num_joints(self):
        return len(self._p)

    def parents(self):
        return self._p


class _Dataset:
    def __init__(self, parents):
        self._s = _Skeleton(parents)

    def skeleton(self):
        return self._s


def test_gcn_model_pos_preparation(built, tmp_path, capsys):
    from dhaug_amd.function_baseline.model_pos_preparation import (POSENETS, gcn_model_pos_preparation, model_pos_preparation,
                                                                   multi_frame_model_pos_preparation)
    from dhaug_amd.models_baseline.gcn import SemGCN
    args = argparse.Namespace(posenet_name="gcn", stages=2, pretrain=False, dropout=0.25, architecture="3,3")
    m = gcn_model_pos_preparation(args, None, torch.device("cpu"))
    assert isinstance(m, SemGCN) and len(m.gconv_layers) == 2 and m.hid_dim == 128 and m.gconv_input[0].dropout.p == 0.25
    assert "parameters" in capsys.readouterr().out
    m2 = gcn_model_pos_preparation(args, _Dataset(CU.PARENTS), torch.device("cpu"), flag="test")
    assert (m2.gconv_output.rows, m2.gconv_output.cols) == CU.pattern()
    args.stages = 4
    assert sum(p.numel() for p in gcn_model_pos_preparation(args, _Dataset(CU.PARENTS), torch.device("cpu")).parameters()) == 267343
    # a checkpoint
    state = CU.seeded_state(128, 1, 3)
    path = str(tmp_path / "ckpt.pth.tar")
    torch.save({"model_pos": state}, path)
    args = argparse.Namespace(posenet_name="gcn", stages=1, pretrain=True, dropout=0.25, posenet_pretrain_path=path)
    m = gcn_model_pos_preparation(args, None, torch.device("cpu"))
    assert all(torch.equal(a, state[k]) for k, a in m.state_dict().items())
    args.posenet_pretrain_path = None
    with pytest.raises(ValueError, match="posenet_pretrain_path"):
        gcn_model_pos_preparation(args, None, torch.device("cpu"))
    # other names; and the two older factories still refuse this one
    args = argparse.Namespace(posenet_name="gcn", stages=2, pretrain=False, dropout=0.25, architecture="3,3")
    for name in ("mlp", "videopose", "mulit_farme_videopose", "mulit_farme_poseformer", "nonsense"):
        args.posenet_name = name
        with pytest.raises(NotImplementedError, match="gcn"):
            gcn_model_pos_preparation(args, None, torch.device("cpu"))
    args.posenet_name = "gcn"
    assert POSENETS == ("videopose",)
    with pytest.raises(NotImplementedError, match="videopose"):
        model_pos_preparation(args, None, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="mulit_farme_videopose"):
        multi_frame_model_pos_preparation(args, None, torch.device("cpu"))


def test_construction_errors(built):
    from dhaug_amd.models_baseline.gcn import SemGCN, SemGraphConv, adj_mx_from_parents
    adj = CU.adj_matrix()
    with pytest.raises(ValueError, match="multiple of 16"):
        SemGCN(adj, 40)
    with pytest.raises(ValueError, match="multiple of 16"):
        SemGCN(adj, 8)
    with pytest.raises(NotImplementedError, match="nodes_group"):
        SemGCN(adj, 32, nodes_group=[[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="16 x 16"):
        SemGCN(adj_mx_from_parents([-1, 0, 1]), 32)
    with pytest.raises(ValueError, match="square"):
        SemGraphConv(2, 4, torch.ones(3, 4))
    with pytest.raises(ValueError, match="parent"):
        adj_mx_from_parents([-1, 5])
    m = make(built, CU.SMALL)
    m.gconv_layers[0].gconv2.bn.momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        m(torch.zeros(2, 16, 2))
    m = make(built, CU.SMALL)
    m.precision = "f16x3"
    assert m._arithmetic() == "bf16x6"
    # a SemGraphConv on its own is the layer in plain torch (no bias: the reference's bias=False)
    g = SemGraphConv(2, 4, adj, bias=False)
    x = torch.randn(3, 16, 2)
    assert g.bias is None and torch.allclose(g(x), CU.mix_ref(x @ g.W[0], x @ g.W[1], CU.softmax_adjacency(g.e)), atol=1e-6)


def test_graph_argument_errors(built):
    """the graph entry points (csrc/dhaug_graph.hip): a bad argument comes back as the documented code before any launch -- every
    pointer here is a valid HOST address, so a call that got as far as a launch would return a HIP error -- and an empty problem is
    a no-op that looks at no pointer"""
    L = built._lib.lib()
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c = ctypes.c_void_p(base), ctypes.c_void_p(base + 8192), ctypes.c_void_p(base + 16384)
    odd4, odd2 = ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)
    EINVAL, EALIGN, EUNSUP = -1, -2, -3

    def mix(src=a, sb=0, lds=32, A=b, bias=None, dst=c, db=0, ldd=16, M=16, C=16, tr=0):
        return L.dhaug_graph_mix(src, sb, lds, A, bias, dst, db, ldd, M, C, tr, None)

    assert mix(src=None) == EINVAL and mix(A=None) == EINVAL and mix(dst=None) == EINVAL
    assert mix(sb=2) == EINVAL and mix(db=-1) == EINVAL and mix(tr=2) == EINVAL and mix(M=-16) == EINVAL and mix(C=-1) == EINVAL
    assert mix(M=17) == EINVAL and mix(M=8) == EINVAL                     # 16 rows per pose
    assert mix(tr=1, lds=16, ldd=32, bias=b) == EINVAL                    # the adjoint has no bias
    assert mix(lds=31) == EALIGN and mix(ldd=15) == EALIGN                # short leading dimensions
    assert mix(tr=1, lds=15, ldd=32) == EALIGN and mix(tr=1, lds=16, ldd=31) == EALIGN
    assert mix(db=1, C=24, lds=48, ldd=24) == EALIGN                      # bf16 rows shorter than ceil16(C)
    assert mix(tr=1, db=1, sb=1, C=20, lds=20, ldd=40) == EALIGN          # ... than ceil16(2C)
    assert mix(src=odd2) == EALIGN and mix(dst=odd2) == EALIGN and mix(A=odd2) == EALIGN and mix(bias=odd2) == EALIGN
    assert mix(C=1 << 28, lds=1 << 29, ldd=1 << 28) == EUNSUP
    assert mix(M=0, src=None, A=None, dst=None) == 0 and mix(C=0, src=None, A=None, dst=None) == 0

    def adj(g=a, gb=0, ldg=16, h=a, hb=0, ldh=32, pairs=b, nnz=4, dA=c, ws=c, M=16, C=16):
        return L.dhaug_graph_adj_grad(g, gb, ldg, h, hb, ldh, pairs, nnz, dA, ws, M, C, None)

    assert adj(g=None) == EINVAL and adj(h=None) == EINVAL and adj(pairs=None) == EINVAL and adj(dA=None) == EINVAL
    assert adj(ws=None) == EINVAL and adj(gb=2) == EINVAL and adj(hb=-1) == EINVAL and adj(M=24) == EINVAL and adj(M=-16) == EINVAL
    assert adj(nnz=-1) == EINVAL and adj(nnz=257) == EINVAL
    assert adj(ldg=15) == EALIGN and adj(ldh=31) == EALIGN
    assert adj(g=odd2) == EALIGN and adj(h=odd2) == EALIGN and adj(pairs=odd2) == EALIGN and adj(dA=odd2) == EALIGN
    assert adj(ws=odd4) == EALIGN
    assert adj(C=1 << 28, ldg=1 << 28, ldh=1 << 29) == EUNSUP
    assert adj(M=0, g=None, h=None, pairs=None, dA=None, ws=None) == 0 and adj(C=0, g=None, h=None, dA=None, ws=None) == 0

    def wcat(src=a, dst=c, n_in=4, n_out=8, to_cat=1):
        return L.dhaug_graph_wcat(src, dst, n_in, n_out, to_cat, None)

    assert wcat(src=None) == EINVAL and wcat(dst=None) == EINVAL and wcat(dst=a) == EINVAL and wcat(to_cat=2) == EINVAL
    assert wcat(n_in=-1) == EINVAL and wcat(n_out=-1) == EINVAL
    assert wcat(src=odd2) == EALIGN and wcat(dst=odd2) == EALIGN
    assert wcat(n_in=1 << 28) == EUNSUP and wcat(n_in=1 << 16, n_out=1 << 16) == EUNSUP
    assert wcat(n_in=0, src=None, dst=None) == 0 and wcat(n_out=0, src=None, dst=None) == 0


def test_launch_constants_mirror_the_sources(built):
    """tests/gcn_util's launch constants are the kernels' (the multi-pass sizes of the GPU tests are derived from them), and the
    Python layer's workspace size is the header's"""
    src = open(os.path.join(PKG, "csrc", "dhaug_graph.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert int(re.search(r"constexpr int kMixBlock = (\d+);", src).group(1)) == CU.MIX_BLOCK
    assert int(re.search(r"constexpr int kJoints = (\d+);", src).group(1)) == CU.JOINTS
    assert "kMixMaxBlocks = DHAUG_GRAPH_MIX_MAX_BLOCKS" in src and "kAdjMaxBlocks = DHAUG_GRAPH_ADJ_MAX_BLOCKS" in src
    assert define("DHAUG_GRAPH_MIX_MAX_BLOCKS") == CU.MIX_MAX_BLOCKS
    assert define("DHAUG_GRAPH_ADJ_MAX_BLOCKS") == CU.ADJ_MAX_BLOCKS
    assert define("DHAUG_GRAPH_MAX_PAIRS") == CU.MAX_PAIRS == built._lib.GRAPH_MAX_PAIRS
    assert re.search(r"#define\s+DHAUG_GRAPH_ADJ_WORKSPACE_DOUBLES\s+\(DHAUG_GRAPH_ADJ_MAX_BLOCKS \* DHAUG_GRAPH_MAX_PAIRS\)", hdr)
    assert built._lib.GRAPH_ADJ_WORKSPACE_DOUBLES == CU.ADJ_MAX_BLOCKS * CU.MAX_PAIRS
    # the sizes the GPU tests derive: C = 4 fp32 is one item per pose
    assert CU.mix_items(1, 4, torch.float32, False) == 1 and CU.mix_items(1, 128, torch.float32, False) == 32
    assert CU.mix_items(1, 128, torch.bfloat16, True) == 16 and CU.mix_items(1, 24, torch.bfloat16, True) == 4
    assert CU.mix_items(1, 20, torch.bfloat16, True, transpose=True) == 4 and CU.mix_items(3, 3, torch.float32, False, True) == 3
