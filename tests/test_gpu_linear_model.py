"""GPU tests of the MLP posenet (models_baseline/mlp/linear_model.py) and of dhaug_bn_fold_bias against the reference's fp64 records
(tests/golden/posenet_mlp.npz), the stock-torch container of the same names on the same device, and itself (launch accounting, the
evaluation cache, weight-cache staleness, dropout).  Every test prints its figures ("FIGURE ...") before it asserts.

The error of a tensor is max|t - ref| / max|ref|.  The floor N of a record is what the stock module (nn.Linear / nn.BatchNorm1d,
fp32, linear_model_util.StockMLP) gives on this GPU against the same fp64 record, worst tensor; the 'bf16x6' module must stay
within 4 N (this project's standing allowance for another summation order).  The gradient of a bias in front of a training-mode
BatchNorm is left out of both sides' figures: the record holds ~1e-17 there, stock fp32 rounding residue, and ours must be
exactly zero (None, or a zero slot of the optimizer's flat gradient)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import golden_util as GU
import linear_model_util as LU
import posetrain_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MEASURED_ON = "2026-10-20, MI355X (gfx950), ROCm PyTorch"
# stock fp32 module against the fp64 record, worst tensor, rounded up (ours, 'bf16x6', on the same run in brackets)
N_A = {96: 1.28e-6, 40: 9.9e-7}         # measured 1.272e-06 (1.021e-06), 9.896e-07 (8.853e-07)
N_B = 1.58e-6                           # measured 1.579e-06 (3.830e-06, grad_linear_stages.1.w2.weight: 2.4 N; deterministic, no atomics)
N_RAGGED = 5.2e-7                       # measured 5.188e-07 (6.624e-07); linear_size 40, one stage, 33 rows, against the fp64 restatement
# record (c), the 12-step fp64 loop: stock torch on this GPU WITH ITS PRE-BN BIASES FROZEN (absolute on the state, relative on the rest)
N_LOOP = dict(param=8.2e-7, loss=1.89e-7, norm=2.23e-7)       # measured 8.124e-07 (5.442e-07), 1.884e-07 (1.702e-07), 2.229e-07 (2.229e-07)
# the same loop with the stock container's pre-BN biases free (stock fp32 torch as it is): state 4.875e-03, loss and norm as frozen --
# a printed figure, asserted nowhere: it documents why such a bias is a constant here
# 'bf16' / 'bf16x3' are NOT parity modes; they are held to 4 x the stock container in torch.bfloat16, measured in the test itself.
# Measured (ours 'bf16' / 'bf16x3' / stock bfloat16): (a) out 4.8e-3 / 5.7e-6 / 5.3e-3, loss 9.4e-5 / 7.8e-7 / 1.8e-3, worst gradient
# tensor 0.21 / 2.2e-5 / 0.19, buffers 1.7e-3 / 2.5e-6 / 4.0e-3; (b) out 5.8e-3 / 9.4e-6 / 6.0e-3, loss 2.8e-4 / 1.1e-7 / 9.0e-4,
# gradient 0.40 / 2.5e-2 / 0.37, buffers 1.3e-3 / 2.2e-6 / 3.1e-3


def figure(name, value):
    print("FIGURE %s %.4g" % (name, value))


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    from dhaug_amd import autograd_ops
    from dhaug_amd.function_aug import model_pos_eval, model_pos_train
    from dhaug_amd.models_baseline.mlp import LinearModel
    from dhaug_amd.models_baseline.videopose import model_VideoPose3D
    return argparse.Namespace(pkg=dhaug_amd, T=model_pos_train, E=model_pos_eval, Model=LinearModel, lib=dhaug_amd._lib,
                              ops=dhaug_amd.ops, A=autograd_ops, V=model_VideoPose3D)


@pytest.fixture(scope="module")
def G():
    return LU.load_golden(LU.GOLDEN)


def state_of(cfg):
    return LU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"])


def make(D, cfg, prec, dropout=0.0, state=None):
    m = D.Model(32, 45, linear_size=cfg["C"], num_stage=cfg["stages"], p_dropout=dropout)
    m.load_state_dict(state_of(cfg) if state is None else state, strict=True)
    m.precision = prec
    return m.cuda()


def make_stock(cfg, dtype=torch.float32):
    m = LU.StockMLP(cfg["C"], cfg["stages"])
    m.load_state_dict(state_of(cfg), strict=True)
    return m.cuda().to(dtype)


def evaluate(m, x):
    m.eval()
    with torch.no_grad():
        return m(x)


class Calls:
    """the names of the C-ABI calls made inside the block"""

    def __init__(self, D):
        self.D, self.names = D, []

    def __enter__(self):
        self.orig = self.D.lib.call

        def counting(name, *a):
            self.names.append(name)
            return self.orig(name, *a)

        self.D.lib.call = counting
        return self

    def __exit__(self, *exc):
        self.D.lib.call = self.orig

    def count(self, name):
        return sum(1 for n in self.names if n == name)


# ---------------------------------------------------------------------------------------------------------------- the fold kernel
@pytest.mark.parametrize("N,K", [(1, 1), (48, 40), (45, 1024), (1024, 1024)])
def test_bn_fold_bias_kernel(D, N, K):
    """b' within one fp32 ulp at |beta| + |(b - rm) gamma rstd| of the fp64 value (formed in fp64 and rounded once: half an ulp of
    the result, which is no larger than that sum); W' and rstd bit-equal to dhaug_bn_fold's; and with a NULL layer bias the entry
    point gives dhaug_bn_fold's bits in every output"""
    g = torch.Generator().manual_seed(100 * N + K)
    r = lambda *s: torch.rand(*s, generator=g)
    W = ((r(N, K) * 2 - 1) / K ** 0.5).cuda()
    gamma, beta, lb = (r(N) + 0.5).cuda(), ((r(N) * 2 - 1) * 0.25).cuda(), ((r(N) * 2 - 1) * LU.BIAS_SCALE).cuda()
    rm, rv, eps = ((r(N) * 2 - 1) * 0.5).cuda(), (r(N) * 1.5 + 0.5).cuda(), 1e-5
    W0, b0, r0 = D.ops.bn_fold(W, gamma, beta, rm, rv, eps)
    with Calls(D) as c:
        W1, b1, r1 = D.ops.bn_fold(W, gamma, beta, rm, rv, eps, layer_bias=lb)
    assert c.names == ["dhaug_bn_fold_bias"]
    assert torch.equal(W1, W0) and torch.equal(r1, r0)
    rs = 1.0 / torch.sqrt(rv.double() + float(np.float32(eps)))
    shift = (lb.double() - rm.double()) * gamma.double() * rs
    want = beta.double() + shift
    err = ((b1.double() - want).abs() / LU.ulp32(beta.double().abs() + shift.abs())).max().item()
    moved = (b1 - b0).abs().max().item()
    figure("fold_bias_%dx%d_ulps" % (N, K), err), figure("fold_bias_%dx%d_bias_term" % (N, K), moved)
    assert err <= 1.0
    assert N == 1 or moved > 0.05                    # (the layer bias is in the result)
    assert ((r0.double() - rs).abs() <= LU.ulp32(rs)).all()
    # without the weight (a block's second layer), and the NULL bias through the C ABI
    W2, b2, r2 = D.ops.bn_fold(None, gamma, beta, rm, rv, eps, want_weight=False, layer_bias=lb)
    assert W2 is None and torch.equal(b2, b1) and torch.equal(r2, r1)
    Wn, bn, rn = torch.full_like(W, 7.0), torch.full_like(b0, 7.0), torch.full_like(r0, 7.0)
    p = lambda t: t.data_ptr()
    D.lib.call("dhaug_bn_fold_bias", p(W), K, None, p(gamma), p(beta), p(rm), p(rv), eps, p(Wn), K, p(bn), p(rn), N, K,
               torch.cuda.current_stream().cuda_stream)
    assert torch.equal(Wn, W0) and torch.equal(bn, b0) and torch.equal(rn, r0)


# ---------------------------------------------------------------------------------------------------------------- parity
def run_record(m, cfg, M, dtype=torch.float32):
    """what the fixture's records hold, in their order: out, loss, grad_*, buf_*, eval_out"""
    x, t = LU.make_inputs(M, cfg["seed"] + 100 + M)
    x, t = x.cuda().to(dtype), t.cuda().to(dtype)
    m.train()
    out = m(x)
    loss = nn.functional.mse_loss(out, t)
    loss.backward()
    rec = [("out", out.detach()), ("loss", loss.detach().reshape(1))]
    rec += [("grad_" + k, p.grad) for k, p in m.named_parameters()]
    rec += [("buf_" + k, b.detach().clone()) for k, b in m.named_buffers()]
    m.eval()
    with torch.no_grad():
        rec.append(("eval_out", m(x)))
    return rec


def compact_ref(G, n):
    keys = [k for k in G if k.startswith("b_f64_%s__" % n)]
    return {k.rsplit("__", 1)[1]: torch.from_numpy(np.array(G[k])) for k in keys}


def errors(rec, G, which, M, cfg, ours):
    """per tensor: record (a) whole tensors; record (b) the figure golden_util.compact_close bounds (sampled elements relative to
    the largest sample, projections / (4 sqrt n)).  ours: the pre-BN bias gradients must be exactly zero; they are in no figure"""
    pre = ["grad_" + k for k in LU.pre_bn_biases(cfg["stages"])]
    out = {}
    for i, (n, v) in enumerate(rec):
        if n in pre:
            if ours:
                assert v is None or not v.any(), n
            continue
        if "num_batches" in n:
            assert int(v) == int(G["a%d_f64_%s" % (M, n)] if which == "a" else G["b_f64_" + n]) == 1, n
            continue
        if which == "a":
            ref = torch.from_numpy(np.array(G["a%d_f64_%s" % (M, n)]))
            out[n] = (v.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
            continue
        ref, got = compact_ref(G, n), GU.compact(v, i)
        key = "full" if "full" in ref else "sample"
        scale = ref[key].abs().max().item()
        e = (got[key].double() - ref[key].double()).abs().max().item() / scale
        if "proj" in ref:
            e = max(e, (got["proj"] - ref["proj"].double()).abs().max().item() / (4.0 * scale * v.numel() ** 0.5))
        out[n] = e
    assert not any(e != e for e in out.values())
    return out


def parity(D, G, which, cfg, M, floor):
    e_stock = errors(run_record(make_stock(cfg), cfg, M), G, which, M, cfg, False)
    e_ours = errors(run_record(make(D, cfg, "bf16x6"), cfg, M), G, which, M, cfg, True)
    layers = 2 * cfg["stages"] + 1
    assert len(e_ours) == len(e_stock) == 3 + (3 * layers + 2) + 2 * layers
    worst = max(e_ours, key=e_ours.get)
    tag = "%s%s" % (which, M if which == "a" else "")
    figure(tag + "_stock_floor", max(e_stock.values())), figure(tag + "_ours", e_ours[worst])
    print("worst tensor:", worst, "stock's:", max(e_stock, key=e_stock.get))
    assert max(e_stock.values()) <= 4 * floor, "the recorded floor no longer describes stock torch on this device"
    for n, e in e_ours.items():
        assert e <= 4 * floor, (n, e)


@pytest.mark.parametrize("M", LU.ROWS_A)
def test_parity_record_a(D, G, M):
    """C = 64, stages 2: whole tensors, no element left out"""
    parity(D, G, "a", LU.SMALL, M, N_A[M])


def test_parity_record_b(D, G):
    """C = 1 024, stages 2, through golden_util.compact records (every recorded sample and projection)"""
    parity(D, G, "b", LU.WIDE, LU.ROWS_B, N_B)


def test_smallest_ragged_shape(D):
    """linear_size 40 (no multiple of 16: padded bf16 rows, ragged GEMM tiles and BatchNorm strips), one stage, 33 rows: forward,
    backward, buffers and evaluation against the fp64 restatement, the same 4 N rule with stock torch on this shape as N"""
    cfg, M = LU.RAGGED, LU.ROWS_RAGGED
    x, t = LU.make_inputs(M, cfg["seed"] + 100 + M)
    ref = LU.network_ref(state_of(cfg), x, t)
    want = dict(out=ref["out"], loss=ref["loss"].reshape(1), eval_out=ref["eval_out"])
    want.update({"grad_" + k: v for k, v in ref["grads"].items()})
    want.update({"buf_" + k: v for k, v in ref["buffers"].items()})
    pre = ["grad_" + k for k in LU.pre_bn_biases(cfg["stages"])]

    def errs(m, ours):
        out = {}
        for n, v in run_record(m, cfg, M):
            if n in pre:
                assert not ours or v is None or not v.any(), n
            elif "num_batches" in n:
                assert int(v) == 1
            else:
                assert v.shape == want[n].shape and not torch.isnan(v).any(), n
                out[n] = (v.double().cpu() - want[n]).abs().max().item() / want[n].abs().max().item()
        return out

    e_stock = errs(make_stock(cfg), False)
    for prec in ("bf16x6", "bf16x3", "bf16"):
        e = errs(make(D, cfg, prec), True)
        assert len(e) == len(e_stock) == 3 + 11 + 6
        figure("ragged_%s" % prec, max(e.values()))
        if prec == "bf16x6":
            figure("ragged_stock_floor", max(e_stock.values()))
            print("worst tensor:", max(e, key=e.get))
            assert max(e_stock.values()) <= 4 * N_RAGGED, "the recorded floor no longer describes stock torch on this device"
            assert max(e.values()) <= 4 * N_RAGGED, e


# ---------------------------------------------------------------------------------------------------------------- the loop
def loop_batches():
    p3, p2 = LU.train_data()
    B = LU.TRAIN["batch"]
    return [(p3[i:i + B], p2[i:i + B]) for i in range(0, LU.TRAIN["n"], B)]


def loop_diffs(model, losses, norms, G):
    sd = model.state_dict()
    d_param = max((sd[k].double().cpu() - torch.from_numpy(np.array(G["c_final_" + k])).double()).abs().max().item()
                  for k in sd if sd[k].dtype.is_floating_point)
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) / np.asarray(b) - 1).max())
    return d_param, rel(losses, G["c_losses"]), rel(norms, G["c_norms"])


def test_training_loop_record_c(D, G):
    """train_posenet + posenet_optimizer in 'bf16x6' on record (c)'s data against the reference's loop RUN IN FP64: final state
    (absolute), per-step losses and gradient norms (relative) within 4 N, N being the stock container on this GPU with its pre-BN
    biases frozen.  The stock container with those biases free -- stock fp32 torch as it is -- is printed, not asserted: Adam
    turns their rounding-residue gradients into steps of ~lr (3.7e-3 on the CPU), which is why it is no yardstick for a loop."""
    cfg = LU.SMALL
    to_dev = [(a.cuda(), b.cuda()) for a, b in loop_batches()]
    d_stock = {}
    for frozen in (True, False):
        stock = make_stock(cfg)
        for b in stock.pre_bn_biases():
            b.requires_grad_(not frozen)
        opt = torch.optim.Adam([p for p in stock.parameters() if p.requires_grad], lr=LU.TRAIN["lr"])
        s_losses, s_norms = PU.stock_loop(stock, "single", to_dev, opt, nn.MSELoss(reduction="mean"))
        d_stock[frozen] = loop_diffs(stock, s_losses.cpu().numpy(), s_norms.cpu().numpy(), G)
    model = make(D, cfg, "bf16x6")
    first = {k: v.clone() for k, v in model.state_dict().items()}
    D.T.train_posenet(model, PU.loader_of("single", loop_batches()), D.T.posenet_optimizer(model, LU.TRAIN["lr"]),
                      nn.MSELoss(reduction="mean"), torch.device("cuda"), PU.loop_args())
    trace = D.T.train_posenet.last_trace.cpu().double().numpy()
    assert len(trace) == 12 == len(G["c_losses"])
    d_ours = loop_diffs(model, trace[:, 0], trace[:, 1], G)
    for name, s, f, o in zip(("param", "loss", "norm"), d_stock[True], d_stock[False], d_ours):
        figure("c_stock_frozen_" + name, s), figure("c_stock_free_" + name, f), figure("c_ours_" + name, o)
    sd = model.state_dict()
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 12, k
        elif k in LU.pre_bn_biases(cfg["stages"]):
            assert torch.equal(sd[k], first[k]), k
        else:
            assert not torch.equal(sd[k], first[k]), k
    for name, s, o in zip(("param", "loss", "norm"), d_stock[True], d_ours):
        assert s <= 4 * N_LOOP[name], ("stock floor", name, s)
        assert o <= 4 * N_LOOP[name], (name, o)


# ---------------------------------------------------------------------------------------------------------------- launches
@pytest.mark.parametrize("prec", ["bf16", "bf16x3", "bf16x6"])
def test_training_step_launches(D, prec):
    """a training step is the VideoPose class's step at the same width and depth, call for call: a bias in front of a BatchNorm
    costs no launch (no dhaug_colsum_* beyond the output bias's, no extra GEMM), its gradient is None after backward, its slot of
    the optimizer's flat gradient is exactly zero, and the optimizer step leaves its bits alone"""
    cfg = LU.SMALL
    x, t = LU.make_inputs(96, 5)
    x, t = x.cuda(), t.cuda()
    sibling = D.V.TemporalModelOptimized1f(16, 2, 15, [1] * (cfg["stages"] + 1), dropout=0.0, channels=cfg["C"]).cuda()
    sibling.precision = prec
    model = make(D, cfg, prec)
    names = []
    for m in (sibling, model):
        m.train()
        opt = D.T.posenet_optimizer(m, 1e-2)
        before = {k: v.clone() for k, v in m.state_dict().items()}
        with Calls(D) as c:
            out = m(x)
            opt.zero_grad()
            nn.functional.mse_loss(out, t).backward()
        names.append(c.names)
        if m is model:
            pre = LU.pre_bn_biases(cfg["stages"])
            params = dict(m.named_parameters())
            assert all(params[k].grad is None for k in pre) and all(p.grad is not None for k, p in params.items() if k not in pre)
            opt.clip_step(1)
            torch.cuda.synchronize()
            for p, gv in zip(opt._params, opt._views):
                zero = not gv.any().item()
                assert zero == any(p is params[k] for k in pre)
            after = m.state_dict()
            assert all(torch.equal(after[k], before[k]) == (k in pre) for k in after if after[k].dtype.is_floating_point)
    colsums = [n for n in names[1] if n.startswith("dhaug_colsum")]
    figure("train_step_calls_" + prec, len(names[1])), figure("train_step_colsums_" + prec, len(colsums))
    assert names[1] == names[0]
    assert len(colsums) <= 1
    assert sum(1 for n in names[1] if n == "dhaug_bn_act_backward") == 2 * cfg["stages"] + 1


def test_evaluation_cache(D):
    """the first evaluation forward folds every hidden layer through dhaug_bn_fold_bias (dhaug_bn_fold never); the second folds,
    casts, splits and packs no WEIGHT (in 'bf16' the one cast left is the network input's) and gives the same bits;
    load_state_dict, a change of one pre-BN bias alone, an optimizer step and a training forward each redo the fold, and the
    output is a fresh module's"""
    cfg = LU.SMALL
    x = LU.make_inputs(40, 8)[0].cuda()
    layers = 2 * cfg["stages"] + 1
    for prec, per_forward in (("bf16", {"dhaug_cast_pad_bf16": 1}), ("bf16x6", {"dhaug_split_bf16": layers + 1})):
        model = make(D, cfg, prec).eval()

        def forward():
            with Calls(D) as c:
                with torch.no_grad():
                    y = model(x)
            weight_side = sum(c.count(n) - per_forward.get(n, 0) for n in ("dhaug_cast_pad_bf16", "dhaug_split_bf16", "dhaug_cast_transpose_bf16"))
            assert c.count("dhaug_bn_fold") == 0 and not [n for n in c.names if "pack" in n]
            return y, c.count("dhaug_bn_fold_bias"), weight_side, c

        def refolded(what):
            y, folds, prepared, _ = forward()
            assert folds == layers and prepared == layers + 1, what
            assert torch.equal(y, evaluate(make(D, cfg, prec, state=model.state_dict()), x)), what
            y2, folds, prepared, _ = forward()
            assert folds == 0 and prepared == 0 and torch.equal(y, y2), what
            return y

        y1, folds, prepared, _ = forward()
        assert folds == layers and prepared == layers + 1
        y2, folds, prepared, c = forward()
        assert folds == 0 and prepared == 0 and torch.equal(y1, y2)
        assert c.count("dhaug_gemm_bf16") == layers + 1
        assert c.count("dhaug_bn_act_forward") == cfg["stages"] and c.count("dhaug_bn_partials") == 0
        model.load_state_dict(LU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"] + 1))
        y3 = refolded("load_state_dict")
        assert not torch.equal(y3, y1)
        for bias in (model.w1.bias, model.linear_stages[1].w2.bias):         # (a folded layer's, and a residual layer's own GEMM bias)
            with torch.no_grad():
                bias.add_(0.5)
            y4 = refolded("a pre-BN bias alone")
            assert not torch.equal(y4, y3)
            y3 = y4
        model.train()
        opt = D.T.posenet_optimizer(model, 1e-2)
        opt.zero_grad()
        model(x).square().mean().backward()
        opt.clip_step(1)
        model.eval()
        y5 = refolded("an optimizer step")
        model.train()
        with torch.no_grad():
            model(x)
        model.eval()
        y6 = refolded("a training forward")
        assert not torch.equal(y6, y5)


def test_optimizer_step_invalidates_packed_weights(D):
    """two PosenetAdam steps in 'bf16' (whose GEMMs read bf16 copies of the weights cached on the parameters): the second step's
    forward equals, bit for bit, the forward of a freshly constructed module loaded with the stepped state"""
    cfg = LU.SMALL
    model = make(D, cfg, "bf16").train()
    opt = D.T.posenet_optimizer(model, 1e-2)
    x, t = LU.make_inputs(96, 5)
    x, t = x.cuda(), t.cuda()
    for step in range(2):
        state = {k: v.clone() for k, v in model.state_dict().items()}
        out = model(x)
        if step == 1:
            fresh = make(D, cfg, "bf16", state=state).train()
            assert torch.equal(out.detach(), fresh(x).detach()), "the forward after an optimizer step read stale packed weights"
        opt.zero_grad()
        nn.functional.mse_loss(out, t).backward()
        opt.clip_step(1)
    assert not torch.equal(model.state_dict()["w1.weight"], state["w1.weight"])


# ---------------------------------------------------------------------------------------------------------------- throughput modes
def summary(e):
    worst = lambda prefix: max(v for k, v in e.items() if k.startswith(prefix))
    return dict(out=e["out"], loss=e["loss"], grad=worst("grad_"), buffers=worst("buf_"), eval_out=e["eval_out"])


@pytest.mark.parametrize("which", ["a", "b"])
def test_throughput_modes_are_not_parity(D, G, which):
    """'bf16' and 'bf16x3' are throughput modes, NOT parity modes: output, loss, worst gradient tensor and buffers each within 4 x
    what the stock container run in torch.bfloat16 on this GPU gives against the same fp64 record"""
    cfg, M = (LU.SMALL, 96) if which == "a" else (LU.WIDE, LU.ROWS_B)
    stock = summary(errors(run_record(make_stock(cfg, torch.bfloat16), cfg, M, torch.bfloat16), G, which, M, cfg, False))
    ours = {prec: summary(errors(run_record(make(D, cfg, prec), cfg, M), G, which, M, cfg, True)) for prec in ("bf16", "bf16x3")}
    for k in ("out", "loss", "grad", "buffers", "eval_out"):
        figure("%s_stock_bfloat16_%s" % (which, k), stock[k])
        for prec in ours:
            figure("%s_%s_%s" % (which, prec, k), ours[prec][k])
    for prec in ours:
        for k in ("out", "loss", "grad", "buffers"):
            assert ours[prec][k] <= 4 * stock[k], (prec, k, ours[prec][k], stock[k])


# ---------------------------------------------------------------------------------------------------------------- dropout, the rest
def test_dropout(D):
    """the mask follows the device generator (one seed, one mask; consecutive calls differ), p = 0 draws nothing, and at p = 0.5
    the kept share of the first layer's active elements (256 x 64 Bernoulli(0.5) draws less the ReLU's zeros) lies within five
    standard deviations of 0.5 -- a binomial bound"""
    cfg = LU.SMALL
    x = LU.make_inputs(256, 6)[0].cuda()
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    layers = 2 * cfg["stages"] + 1
    first = {}
    orig = D.A.bn_act
    for p in (0.0, 0.5):
        model = make(D, cfg, "bf16x6", dropout=p).train()
        seen = []

        def recording(*a, **k):
            seen.append(orig(*a, **k))
            return seen[-1]

        D.A.bn_act = recording
        try:
            with torch.no_grad():
                torch.manual_seed(5)
                off = gen.get_offset()
                a = model(x)
                drawn = gen.get_offset() - off
                a2 = model(x)
                torch.manual_seed(5)
                b = model(x)
        finally:
            D.A.bn_act = orig
        first[p] = seen[0]
        assert torch.equal(a, b)
        assert drawn == (4 * layers if p else 0)
        assert torch.equal(a, a2) == (p == 0.0)
    active = first[0.0] > 0
    n = int(active.sum())
    kept = int((first[0.5][active] > 0).sum())
    assert not (first[0.5][~active] != 0).any()
    assert torch.equal(first[0.5][active & (first[0.5] > 0)], (first[0.0] * 2.0)[active & (first[0.5] > 0)])
    sd = (0.25 / n) ** 0.5
    figure("dropout_kept_share", kept / n), figure("dropout_sigmas", abs(kept / n - 0.5) / sd)
    assert n > 256 * 64 // 4 and abs(kept / n - 0.5) <= 5 * sd


def test_input_forms_hip_joint_one_row_and_evaluate(D):
    cfg = LU.SMALL
    x, t = LU.make_inputs(64, 7)
    x, t = x.cuda(), t.cuda()
    for prec in ("bf16", "bf16x6"):
        model = make(D, cfg, prec)
        a, b = evaluate(model, x), evaluate(model, x.reshape(64, 32))
        assert a.shape == (64, 16, 3) and torch.equal(a, b) and not a[:, 0].any() and a[:, 1:].abs().min() > 0
        model.train()
        with torch.no_grad():
            state = {k: v.clone() for k, v in model.state_dict().items()}
            c = model(x)
            model.load_state_dict(state)
            d = model(x.reshape(64, 32))
        assert c.shape == (64, 16, 3) and torch.equal(c, d) and not c[:, 0].any()
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            model(x[:1])
        with pytest.raises(ValueError, match=r"\(B, 16, 2\) or \(B, 32\)"):
            model(torch.zeros(4, 17, 2, device="cuda"))
        for bn in (model.batch_norm1, model.linear_stages[0].batch_norm2):
            bn.momentum = None
            with pytest.raises(NotImplementedError, match="momentum=None"):
                model(x)
            bn.momentum = 0.1
        assert evaluate(model, x[:1]).shape == (1, 16, 3)
    model = make(D, cfg, "bf16x6")
    p3 = t + 0.5
    batches = [(p3[i:i + 32], x[i:i + 32]) for i in (0, 32)]
    p1, p2, pck, auc = D.E.evaluate(batches, model, torch.device("cuda"))
    want = (evaluate(model, x).double() - t.double()).norm(dim=-1).mean().item() * 1000.0
    figure("evaluate_p1_mm", p1)
    assert abs(p1 / want - 1) <= 1e-5 and 0 < p2 <= p1
