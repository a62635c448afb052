"""CPU-side checks of the MLP posenet (models_baseline/mlp): the state_dict interface and the seeded initial state against the
reference's records, the plain-torch path against records (a) and (c) of tests/golden/posenet_mlp.npz (fp64) with the biases in
front of a training-mode BatchNorm held constant, the factory, and the argument errors of dhaug_bn_fold_bias (before any launch)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import linear_model_util as LU
import posetrain_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_ROUNDING = 2.0 ** -23          # the least fp32 bound of a tensor: one rounding of its largest element


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def G():
    return LU.load_golden(LU.GOLDEN)


@pytest.fixture(scope="module")
def G32():
    return LU.load_golden(LU.GOLDEN_F32)


def make(built, cfg, dropout=0.0):
    from dhaug_amd.models_baseline.mlp import LinearModel
    m = LinearModel(32, 45, linear_size=cfg["C"], num_stage=cfg["stages"], p_dropout=dropout)
    m.load_state_dict(LU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"]), strict=True)
    return m


def test_state_dict_layout_is_the_references(built, G):
    from dhaug_amd.models_baseline.mlp import Linear, LinearModel
    for C, stages in LU.LAYOUTS:
        m = LinearModel(32, 45, linear_size=C, num_stage=stages, p_dropout=0.25)
        sd, tag = m.state_dict(), "%d_%d" % (C, stages)
        assert list(sd.keys()) == [str(k) for k in G["keys_" + tag]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in G["shapes_" + tag]]
        assert [str(v.dtype) for v in sd.values()] == [str(s) for s in G["dtypes_" + tag]]
        # the test utilities' layout is the same one
        assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [(k, s, d) for k, (s, d) in LU.shapes(C, stages).items()]
    m = LinearModel(32, 45)
    assert sum(p.numel() for p in m.parameters()) == 4288557
    assert (m.linear_size, m.num_stage, m.p_dropout, m.input_size, m.output_size) == (1024, 2, 0.5, 32, 45)
    assert isinstance(m.relu, nn.ReLU) and isinstance(m.dropout, nn.Dropout) and m.dropout.p == 0.5
    blk = m.linear_stages[0]
    assert isinstance(blk, Linear) and blk.l_size == 1024 and isinstance(blk.relu, nn.ReLU) and blk.dropout.p == 0.5
    assert m.precision in ("bf16", "bf16x3", "bf16x6", "f16x3")
    m.precision = "f16x3"
    assert m._arithmetic() == "bf16x6"
    with pytest.raises(ValueError, match="input_size 32"):
        LinearModel(34, 45)


def test_seeded_initial_state_is_the_references(built, G):
    from dhaug_amd.models_baseline.mlp import LinearModel, init_weights
    cfg = LU.INIT
    torch.manual_seed(cfg["seed"])
    m = LinearModel(32, 45, linear_size=cfg["C"], num_stage=cfg["stages"]).apply(init_weights)
    sd = m.state_dict()
    assert len(sd) == 7 * (2 * cfg["stages"] + 1) + 2
    for k, v in sd.items():
        ref = torch.from_numpy(np.array(G["init_" + k]))
        assert v.dtype == ref.dtype and torch.equal(v, ref), k
    lin = nn.Linear(4, 4)
    w, b = lin.weight.clone(), lin.bias.clone()
    init_weights(lin)
    assert not torch.equal(lin.weight, w) and torch.equal(lin.bias, b)
    bn = nn.BatchNorm1d(4)
    init_weights(bn)
    assert torch.all(bn.weight == 1)


def run_cpu(m, M, cfg, dtype):
    x, t = LU.make_inputs(M, cfg["seed"] + 100 + M)
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


@pytest.mark.parametrize("M", LU.ROWS_A)
def test_cpu_path_matches_the_reference_record(built, G, G32, M):
    """record (a): training output, loss, every gradient, the buffers and the evaluation output.  fp64: 1e-10 of each tensor's
    largest element (fp64 against fp64: the summation order differs).  fp32: per tensor, 4 x the distance of the reference class's
    own fp32 run from its fp64 run, computed here from the two records (and no less than 4 x ONE_ROUNDING).  The gradient of a bias in
    front of a BatchNorm is None or exactly zero here (1e-17 in the fp64 record, rounding residue in the fp32 one)."""
    cfg = LU.SMALL
    pre = ["grad_" + k for k in LU.pre_bn_biases(cfg["stages"])]
    names = [k[len("a%d_f64_" % M):] for k in G if k.startswith("a%d_f64_" % M)]
    assert len(names) == 3 + 22 + 15
    runs = {torch.float64: run_cpu(make(built, cfg), M, cfg, torch.float64), torch.float32: run_cpu(make(built, cfg), M, cfg, torch.float32)}
    for dtype, rec in runs.items():
        assert set(rec) == set(names)
        for n in names:
            ref = torch.from_numpy(np.array(G["a%d_f64_%s" % (M, n)]))
            ref32 = torch.from_numpy(np.array(G32["a%d_f32_%s" % (M, n)]))
            if "num_batches" in n:
                assert int(rec[n]) == int(ref) == int(ref32) == 1
                continue
            if n in pre:
                assert rec[n] is None or not rec[n].any(), n
                continue
            assert ref32.dtype == torch.float32 and ref.dtype == torch.float64
            scale = ref.abs().max().item()
            own = (ref32.double() - ref).abs().max().item() / scale
            bound = 1e-10 if dtype == torch.float64 else 4 * max(own, ONE_ROUNDING)
            err = (rec[n].double() - ref).abs().max().item() / scale
            print("FIGURE a%d %s %s err %.3e reference fp32 %.3e" % (M, str(dtype), n, err, own))
            assert err <= bound, (str(dtype), n, err, bound)


def cpu_loop(model, dtype):
    """the reference's sequence of calls on record (c)'s pairs, stock torch pieces, in `dtype`"""
    p3, p2 = LU.train_data()
    B = LU.TRAIN["batch"]
    opt = torch.optim.Adam(model.parameters(), lr=LU.TRAIN["lr"])
    losses, norms = [], []
    model.train()
    for i in range(0, LU.TRAIN["n"], B):
        b3, b2 = p3[i:i + B].to(dtype), p2[i:i + B].to(dtype)
        t = b3 - b3[:, :1]
        for inp, tgt in ((b2, t), (PU.flip(b2).view(len(b2), -1), PU.flip(t))):
            out = model(inp)
            opt.zero_grad()
            loss = nn.functional.mse_loss(out, tgt)
            loss.backward()
            norms.append(float(nn.utils.clip_grad_norm_(model.parameters(), max_norm=1)))
            opt.step()
            losses.append(float(loss.detach()))
    return losses, norms


def test_cpu_loop_matches_the_fp64_record(built, G):
    """record (c), the reference's train_posenet in fp64: the plain-torch path as .double() under torch.optim.Adam reproduces the
    final state, the per-step losses and the gradient norms to 1e-10 of each tensor's largest element, and the biases in front
    of a BatchNorm keep their bits (the record's moved <= 1e-9, asserted by the generator)"""
    cfg = LU.SMALL
    m = make(built, cfg).double()
    first = {k: v.clone() for k, v in m.state_dict().items()}
    losses, norms = cpu_loop(m, torch.float64)
    assert len(losses) == 12 == len(G["c_losses"])
    rel = lambda a, b: float(np.abs(np.asarray(a) / np.asarray(b) - 1).max())
    print("FIGURE c fp64 loss %.3e norm %.3e" % (rel(losses, G["c_losses"]), rel(norms, G["c_norms"])))
    assert rel(losses, G["c_losses"]) <= 1e-10 and rel(norms, G["c_norms"]) <= 1e-10
    sd = m.state_dict()
    for k, v in sd.items():
        ref = torch.from_numpy(np.array(G["c_final_" + k]))
        if not v.dtype.is_floating_point:
            assert int(v) == int(ref) == 12, k
        elif k in LU.pre_bn_biases(cfg["stages"]):
            assert torch.equal(v, first[k]), k
            assert (v - ref).abs().max().item() <= 1e-9, k
        else:
            assert (v - ref).abs().max().item() <= 1e-10 * ref.abs().max().item(), k
            assert not torch.equal(v, first[k]), k


def test_cpu_loop_in_fp32_stays_near_the_fp64_record(built, G):
    """the same loop in fp32: with the biases in front of a BatchNorm constant the state stays fp32-close to the fp64 record, which
    a stock fp32 loop with those biases free does not (Adam's g / (sqrt(v) + eps) turns their rounding-residue gradients into
    steps of ~lr: DESIGN.md section 4.5).  Bounds: the frozen stock loop's own distance x 4 for ours; the free stock loop's
    distance is a printed figure."""
    cfg = LU.SMALL

    def distance(model):
        sd = model.state_dict()
        return max((sd[k].double() - torch.from_numpy(np.array(G["c_final_" + k]))).abs().max().item()
                   for k in sd if sd[k].dtype.is_floating_point)

    def stock(frozen):
        s = LU.StockMLP(cfg["C"], cfg["stages"])
        s.load_state_dict(LU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"]), strict=True)
        if frozen:
            for b in s.pre_bn_biases():
                b.requires_grad_(False)
        s.float()
        p = [q for q in s.parameters() if q.requires_grad]
        opt = torch.optim.Adam(p, lr=LU.TRAIN["lr"])
        s.train()
        p3, p2 = LU.train_data()
        for b3, b2 in [(p3[i:i + 96], p2[i:i + 96]) for i in range(0, 520, 96)]:
            for inp, tgt in PU.steps_of_batch("single", b3, b2):
                out = s(inp)
                opt.zero_grad()
                nn.functional.mse_loss(out, tgt).backward()
                nn.utils.clip_grad_norm_(p, max_norm=1)
                opt.step()
        return distance(s)

    m = make(built, cfg)
    first = {k: v.clone() for k, v in m.state_dict().items()}
    cpu_loop(m, torch.float32)
    ours, frozen, free = distance(m), stock(True), stock(False)
    print("FIGURE c fp32 state distance: ours %.3e stock frozen %.3e stock free %.3e" % (ours, frozen, free))
    assert ours <= 4 * frozen
    assert all(torch.equal(m.state_dict()[k], first[k]) for k in LU.pre_bn_biases(cfg["stages"]))


def test_restatement_matches_the_reference_record(G):
    """tests/linear_model_util.network_ref (the GPU tests' yardstick at the ragged shape) against record (a)"""
    cfg = LU.SMALL
    for M in LU.ROWS_A:
        x, t = LU.make_inputs(M, cfg["seed"] + 100 + M)
        r = LU.network_ref(LU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"]), x, t)
        pairs = [("out", r["out"]), ("loss", r["loss"].reshape(1)), ("eval_out", r["eval_out"])]
        pairs += [("grad_" + k, v) for k, v in r["grads"].items()] + [("buf_" + k, v) for k, v in r["buffers"].items()]
        assert len(pairs) == 3 + 22 + 10
        for n, v in pairs:
            ref = torch.from_numpy(np.array(G["a%d_f64_%s" % (M, n)]))
            if n[5:] in LU.pre_bn_biases(cfg["stages"]):
                assert v.abs().max().item() <= 1e-14 and ref.abs().max().item() <= 1e-14, n
            else:
                assert (v - ref).abs().max().item() <= 1e-10 * ref.abs().max().item(), n


def test_input_forms_hip_joint_and_errors(built):
    m = make(built, LU.SMALL).eval()
    x, _ = LU.make_inputs(7, 5)
    with torch.no_grad():
        a, b = m(x), m(x.reshape(7, 32))
    assert a.shape == (7, 16, 3) and torch.equal(a, b) and torch.all(a[:, 0] == 0) and a[:, 1:].abs().min() > 0
    m.train()
    assert torch.equal(m(x), m(x.reshape(7, 32)))
    for bad in (torch.zeros(4, 17, 2), torch.zeros(4, 31), torch.zeros(4, 2, 16, 2)):
        with pytest.raises(ValueError, match=r"\(B, 16, 2\) or \(B, 32\)"):
            m(bad)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, 16, 2))
    m.eval()
    with torch.no_grad():
        assert m(torch.zeros(1, 16, 2)).shape == (1, 16, 3)


def test_bias_gradient_is_real_in_evaluation_mode(built):
    """evaluation mode with gradients on: BatchNorm uses the running statistics, the bias in front of it has a gradient, and it
    equals the stock container's"""
    cfg = LU.SMALL
    m = make(built, cfg).eval()
    stock = LU.StockMLP(cfg["C"], cfg["stages"]).eval()
    stock.load_state_dict(m.state_dict(), strict=True)
    x, t = LU.make_inputs(9, 3)
    nn.functional.mse_loss(m(x), t).backward()
    nn.functional.mse_loss(stock(x), t).backward()
    for (k, p), q in zip(m.named_parameters(), stock.parameters()):
        assert p.grad is not None and (p.grad - q.grad).abs().max().item() <= 1e-5 * q.grad.abs().max().item(), k
    for k in LU.pre_bn_biases(cfg["stages"]):
        assert dict(m.named_parameters())[k].grad.abs().max().item() > 1e-4, k


def test_state_round_trips_through_stock_modules(built):
    cfg = LU.SMALL
    m = make(built, cfg)
    stock = LU.StockMLP(cfg["C"], cfg["stages"])
    stock.load_state_dict(m.state_dict(), strict=True)
    m2 = make(built, dict(cfg, seed=cfg["seed"] + 1))
    m2.load_state_dict(stock.state_dict(), strict=True)
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    x, _ = LU.make_inputs(7, 5)
    m.eval(), stock.eval()
    with torch.no_grad():
        a, b = m(x), stock(x)
    assert (a - b).abs().max().item() <= 1e-5
    m.train(), stock.train()
    with torch.no_grad():
        assert (m(x) - stock(x)).abs().max().item() <= 1e-5
    for (k, a), b in zip(m.state_dict().items(), stock.state_dict().values()):       # (the running buffers: the bias is in the mean)
        assert (a.double() - b.double()).abs().max().item() <= 1e-6, k


def test_mlp_model_pos_preparation(built, tmp_path, capsys):
    from dhaug_amd.function_baseline import model_pos_preparation as MP
    from dhaug_amd.models_baseline.mlp import LinearModel, init_weights
    assert MP.MLP_POSENETS == ("mlp",) and MP.POSENETS == ("videopose",)
    args = argparse.Namespace(posenet_name="mlp", stages=3, pretrain=False, dropout=0.1)
    torch.manual_seed(4)
    m = MP.mlp_model_pos_preparation(args, None, torch.device("cpu"))
    assert isinstance(m, LinearModel) and m.num_stage == 3 and len(m.linear_stages) == 3 and m.linear_size == 1024
    assert m.dropout.p == 0.1 and m.p_dropout == 0.1 and all(b.dropout.p == 0.1 for b in m.linear_stages)
    assert "mlp: 3 stages" in capsys.readouterr().out
    torch.manual_seed(4)
    want = LinearModel(32, 45, num_stage=3, p_dropout=0.1).apply(init_weights).state_dict()
    assert all(torch.equal(a, want[k]) for k, a in m.state_dict().items())       # init_weights on the host generator
    # the pretrain path
    state = LU.seeded_state(1024, 1, 3)
    path = str(tmp_path / "ckpt.pth.tar")
    torch.save({"model_pos": state}, path)
    args = argparse.Namespace(posenet_name="mlp", stages=1, dropout=0.5, pretrain=True, posenet_pretrain_path=path)
    m = MP.mlp_model_pos_preparation(args, None, torch.device("cpu"))
    assert all(torch.equal(a, state[k]) for k, a in m.state_dict().items())
    args.posenet_pretrain_path = None
    with pytest.raises(ValueError, match="posenet_pretrain_path"):
        MP.mlp_model_pos_preparation(args, None, torch.device("cpu"))
    # every other name is refused, and the other factories keep refusing this one
    args = argparse.Namespace(posenet_name="mlp", stages=2, pretrain=False, dropout=0.25, architecture="3,3")
    for name in ("gcn", "videopose", "mulit_farme_videopose", "mulit_farme_poseformer", "stgcn", "nonsense"):
        with pytest.raises(NotImplementedError, match="mlp"):
            MP.mlp_model_pos_preparation(argparse.Namespace(**dict(vars(args), posenet_name=name)), None, torch.device("cpu"))
    for factory in (MP.model_pos_preparation, MP.multi_frame_model_pos_preparation, MP.gcn_model_pos_preparation):
        with pytest.raises(NotImplementedError, match="mlp"):
            factory(args, None, torch.device("cpu"))
    assert "mlp_model_pos_preparation" in MP.__doc__


def test_bn_fold_bias_argument_errors(built):
    """dhaug_bn_fold_bias (csrc/dhaug_posenet.hip): dhaug_bn_fold's codes, with and without a layer bias -- every pointer here is a
    valid HOST address, so a call that got as far as a launch would return a HIP error -- and N = 0 is a no-op"""
    L = built._lib.lib()
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c = ctypes.c_void_p(base), ctypes.c_void_p(base + 8192), ctypes.c_void_p(base + 16384)
    EINVAL, EALIGN, EUNSUP = -1, -2, -3

    def fold(W=a, ldw=8, lb=b, g=b, bt=b, rm=b, rv=b, eps=1e-5, Wo=c, ldo=8, bo=c, ro=c, N=4, K=8):
        return L.dhaug_bn_fold_bias(W, ldw, lb, g, bt, rm, rv, eps, Wo, ldo, bo, ro, N, K, None)

    for lb in (b, None):
        assert fold(lb=lb, g=None) == EINVAL and fold(lb=lb, rv=None) == EINVAL and fold(lb=lb, bt=None) == EINVAL
        assert fold(lb=lb, rm=None) == EINVAL and fold(lb=lb, W=None) == EINVAL
        assert fold(lb=lb, N=-1) == EINVAL and fold(lb=lb, K=-1) == EINVAL
        assert fold(lb=lb, Wo=None, bo=None, ro=None) == EINVAL and fold(lb=lb, eps=-1.0) == EINVAL
        assert fold(lb=lb, ldw=4) == EALIGN and fold(lb=lb, ldo=4) == EALIGN and fold(lb=lb, g=ctypes.c_void_p(base + 2)) == EALIGN
        assert fold(lb=lb, N=1 << 30) == EUNSUP and fold(lb=lb, K=1 << 30, ldw=1 << 30, ldo=1 << 30) == EUNSUP
        assert fold(lb=lb, N=0, g=None, W=None, Wo=None, bo=None, ro=None) == 0
    assert fold(lb=ctypes.c_void_p(base + 2)) == EALIGN
    assert fold(lb=None, N=0, g=None, W=None, Wo=None, bo=None, ro=None, K=0) == 0
