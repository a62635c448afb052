"""GPU tests of the multi-frame VideoPose posenets (models_Fk_GAN/mulit_farme_videopose.py) against the reference's fp64 records
(tests/golden/posenet_multiframe.npz), the stock-torch containers of the same names on the same device (multiframe_util.
StockMultiFrame) and themselves (weight-cache staleness, the evaluation cache).  Every test prints its figures ("FIGURE ...") before
it asserts.

The error of a tensor is max|t - ref| / max|ref|.  The floor N of a record is what the stock modules (nn.Conv1d / nn.BatchNorm1d,
fp32) give on this GPU against the same fp64 record, worst tensor; the 'bf16x6' modules must stay within 4 N, this project's
standing margin for fp32-grade arithmetic with another summation order.  'bf16' and 'bf16x3' are throughput modes, not parity
modes: their yardstick is the stock network with bf16-rounded parameters, inputs, convolution and activation outputs."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import golden_util as GU
import multiframe_util as MU
import posetrain_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MEASURED_ON = "2026-10-19, MI355X (gfx950), ROCm PyTorch"
# stock fp32 modules against the fp64 record, worst tensor, rounded up (ours, 'bf16x6', on the same run in brackets)
N_A = {"a8_": 6.8e-7, "a5_": 1.11e-6, "a27_4_": 6.18e-6}     # measured 6.763e-07 (5.110e-07), 1.104e-06 (6.040e-07), 6.172e-06 (1.194e-06)
N_B = 1.26e-6                                                 # measured 1.251e-06 (2.056e-06, grad_layers_conv.1.weight: 1.7 N;
                                                              #  7.910e-06 = 6.3 N with the six segments in one launch, see autograd_ops.ORDERED6)
# record (c), the 12-step video loop: stock torch on this GPU against the CPU-recorded loop (absolute on the state, relative on the rest)
N_LOOP = dict(param=2.09e-7, loss=2.09e-7, norm=1.38e-7)      # measured 2.086e-07 (5.290e-07), 2.081e-07 (1.982e-07), 1.378e-07 (1.082e-07)
# throughput modes against the fp64 record a8 (out: of the output's largest element; loss: relative; grad: worst relative L2 of a
# gradient tensor), measured: the bf16 emulation of the stock network, 'bf16', 'bf16x3'.  The test bounds both modes by 4 x the
# emulation's figure of the same run; these are the record of what that run gave.
LOW_MEASURED = dict(emulation=dict(out=5.531e-3, loss=2.232e-4, grad=2.422e-2), bf16=dict(out=5.734e-3, loss=6.302e-4, grad=2.422e-2),
                    bf16x3=dict(out=8.322e-6, loss=1.922e-6, grad=2.027e-5))


def figure(name, value):
    print("FIGURE %s %.4g" % (name, value))


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    from dhaug_amd.function_aug import model_pos_train
    from dhaug_amd.models_Fk_GAN import mulit_farme_videopose, video_mode_operate
    from dhaug_amd.utils import loss
    return argparse.Namespace(pkg=dhaug_amd, T=model_pos_train, V=video_mode_operate, M=mulit_farme_videopose, lib=dhaug_amd._lib,
                              loss=loss)


@pytest.fixture(scope="module")
def G():
    return MU.load_golden()


def make(D, cfg, prec, strided=True, dropout=0.0, state=None, running=False):
    cls = D.M.multiFrame_TemporalModelOptimized1f if strided else D.M.multiFrame_TemporalModel
    m = cls(16, 2, 16, filter_widths=list(cfg["arch"]), dropout=dropout, channels=cfg["C"])
    m.load_state_dict(MU.seeded_state(cfg["C"], cfg["arch"], cfg["seed"], running=running) if state is None else state, strict=True)
    m.precision = prec
    return m.cuda()


def make_stock(cfg, strided=True, running=False, state=None):
    m = MU.StockMultiFrame(cfg["C"], cfg["arch"], strided)
    m.load_state_dict(MU.seeded_state(cfg["C"], cfg["arch"], cfg["seed"], running=running) if state is None else state, strict=True)
    return m.cuda()


def evaluate(m, x):
    m.eval()
    with torch.no_grad():
        return m(x)


def run_record(m, dilated, cfg, B):
    """what the fixture's records hold, in their order: out, loss, grad_*, buf_*, eval_out, dil_out"""
    x, t = MU.record_inputs(cfg, B)
    x, t = x.cuda(), t.cuda()
    m.train()
    out = m(x)
    loss = nn.functional.mse_loss(out, t)
    loss.backward()
    rec = [("out", out.detach()), ("loss", loss.detach().reshape(1))]
    rec += [("grad_" + k, p.grad) for k, p in m.named_parameters()]
    rec += [("buf_" + k, b.detach().clone()) for k, b in m.named_buffers()]
    rec.append(("eval_out", evaluate(m, x)))
    rec.append(("dil_out", evaluate(dilated, MU.dilated_input(cfg).cuda())))
    return rec


def errors_whole(rec, G, prefix):
    out = {}
    for n, v in rec:
        ref = torch.from_numpy(np.array(G[prefix + n]))
        if not ref.dtype.is_floating_point:
            assert int(v) == int(ref), n
            continue
        assert v.shape == ref.shape, n
        out[n] = (v.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    return out


def compact_ref(G, n):
    keys = [k for k in G if k.startswith("b_%s__" % n)]
    return {k.rsplit("__", 1)[1]: torch.from_numpy(np.array(G[k])) for k in keys}


def errors_b(rec, G):
    """the figure compact_close bounds: sampled elements relative to the largest sample, projections / (4 sqrt n)"""
    out = {}
    for i, (n, v) in enumerate(rec):
        if not v.dtype.is_floating_point:
            assert int(v) == int(G["b_" + n]), n
            continue
        ref, got = compact_ref(G, n), GU.compact(v, i)
        key = "full" if "full" in ref else "sample"
        scale = ref[key].abs().max().item()
        e = (got[key].double() - ref[key].double()).abs().max().item() / scale
        if "proj" in ref:
            e = max(e, (got["proj"] - ref["proj"].double()).abs().max().item() / (4.0 * scale * v.numel() ** 0.5))
        out[n] = e
    return out


CASES = [("a%d_" % B, MU.SMALL, B) for B in MU.BATCH_A] + [("a27_%d_" % MU.BATCH_A27, MU.SMALL27, MU.BATCH_A27)]


@pytest.mark.parametrize("prefix,cfg,B", CASES, ids=[c[0] for c in CASES])
def test_parity_records_a(D, G, prefix, cfg, B):
    """C = 64, '3,3' (B = 8 and the ragged 5) and '3,3,3' (B = 4): whole tensors, no element left out; dil_out is the dilated class
    on a (2, receptive field + 7) input with running statistics away from (0, 1)"""
    e_stock = errors_whole(run_record(make_stock(cfg), make_stock(cfg, False, True), cfg, B), G, prefix)
    e_ours = errors_whole(run_record(make(D, cfg, "bf16x6"), make(D, cfg, "bf16x6", False, running=True), cfg, B), G, prefix)
    blocks = len(cfg["arch"]) - 1
    assert len(e_ours) == 4 + (3 + 2 * blocks + 2 * (1 + 2 * blocks)) + 2 * (1 + 2 * blocks)
    worst = max(e_ours, key=e_ours.get)
    figure(prefix + "stock_floor", max(e_stock.values())), figure(prefix + "ours", e_ours[worst])
    figure(prefix + "dil_out_stock", e_stock["dil_out"]), figure(prefix + "dil_out_ours", e_ours["dil_out"])
    print("worst tensor:", worst, "| stock's:", max(e_stock, key=e_stock.get))
    assert max(e_stock.values()) <= 4 * N_A[prefix], "the recorded floor no longer describes stock torch on this device"
    for n, e in e_ours.items():
        assert e <= 4 * N_A[prefix], (n, e)


def test_parity_record_b(D, G):
    """C = 1 024, '3,3', B = 8 (the video command's network), through golden_util.compact records"""
    cfg, B = MU.WIDE, MU.BATCH_B
    e_stock = errors_b(run_record(make_stock(cfg), make_stock(cfg, False, True), cfg, B), G)
    rec = run_record(make(D, cfg, "bf16x6"), make(D, cfg, "bf16x6", False, running=True), cfg, B)
    e_ours = errors_b(rec, G)
    assert len(e_ours) == 4 + 11 + 6
    worst = max(e_ours, key=e_ours.get)
    figure("b_stock_floor", max(e_stock.values())), figure("b_ours", e_ours[worst])
    print("worst tensor:", worst, "| stock's:", max(e_stock, key=e_stock.get))
    for n in sorted(e_ours, key=e_ours.get, reverse=True)[:6]:
        print("FIGURE b %s ours %.3e stock %.3e" % (n, e_ours[n], e_stock[n]))
    assert max(e_stock.values()) <= 4 * N_B, "the recorded floor no longer describes stock torch on this device"
    for i, (n, v) in enumerate(rec):
        if v.dtype.is_floating_point:
            GU.compact_close(v, compact_ref(G, n), i, 0.0, 4 * N_B, n)


def count_calls(D, fn):
    """fn() with the C-ABI calls it makes listed by name"""
    names, orig = [], D.lib.call

    def counting(name, *a):
        names.append(name)
        return orig(name, *a)

    D.lib.call = counting
    try:
        y = fn()
    finally:
        D.lib.call = orig
    return y, names


@pytest.mark.parametrize("prec", ["bf16x6", "bf16"])
def test_dilated_evaluation_slides_the_strided_model(D, prec):
    """(1, T) and (2, T) inputs: the dilated class equals the strided class slid over the sequence frame by frame.  Both sides are
    this package's: in 'bf16x6' each lies within 4 N of the exact network, so they agree within 8 N (N: record a8's floor); in 'bf16'
    the layers round their outputs to bf16 (2^-9 relative), the bound is 2^-5 of the output's largest element -- a guard against a
    wrong window, which is an error of order 1.  The second call packs and folds nothing; a training step of the strided class
    followed by load_state_dict (what video_mode_evaluate_posenet does) makes the operands stale."""
    cfg = MU.SMALL
    rf = MU.receptive_field(cfg["arch"])
    strided, dil = make(D, cfg, prec, running=True), make(D, cfg, prec, False, running=True)
    bound = 8 * N_A["a8_"] if prec == "bf16x6" else 2.0 ** -5
    for B, T in ((1, rf + 11), (2, rf + 4), (1, rf)):
        x = MU.make_inputs(B, T, 40 + T)[0].cuda()
        yd = evaluate(dil, x)
        with torch.no_grad():
            ys = MU.slide(strided.eval(), x)
        assert yd.shape == ys.shape == (B, T - rf + 1, 16, 3)
        err = (yd - ys).abs().max().item() / ys.abs().max().item()
        figure("slide_%s_B%d_T%d" % (prec, B, T), err)
        assert err <= bound, (B, T, err)
    x = MU.make_inputs(1, rf + 11, 77)[0].cuda()
    y1 = evaluate(dil, x)
    y2, names = count_calls(D, lambda: evaluate(dil, x))
    assert torch.equal(y1, y2)
    weight_side = [n for n in names if n in ("dhaug_bn_fold", "dhaug_conv_taps_pack_bf16", "dhaug_conv_taps_permute_f32",
                                             "dhaug_cast_transpose_bf16")]
    assert not weight_side, weight_side
    layers = 1 + 2 * (len(cfg["arch"]) - 1)
    assert sum(1 for n in names if n == "dhaug_gemm_bf16") == (layers + 1) * (2 if prec == "bf16x6" else 1)   # ('bf16x6': two launches per product)
    assert sum(1 for n in names if n == "dhaug_tap_gather") == len(cfg["arch"]) and "dhaug_bn_partials" not in names
    # one training step of the strided class, then its state into the evaluation model
    strided.train()
    opt = D.T.posenet_optimizer(strided, 1e-2)
    xt, t = MU.record_inputs(cfg, 8)
    opt.zero_grad()
    nn.functional.mse_loss(strided(xt.cuda()), t.cuda()).backward()
    opt.clip_step(1)
    dil.load_state_dict(strided.state_dict())
    y3, names = count_calls(D, lambda: evaluate(dil, x))
    assert sum(1 for n in names if n == "dhaug_bn_fold") == layers and not torch.equal(y3, y1)
    fresh = make(D, cfg, prec, False, state={k: v.clone() for k, v in strided.state_dict().items()})
    assert torch.equal(y3, evaluate(fresh, x))


def loop_diffs(model, losses, norms, G):
    sd = model.state_dict()
    diffs = {k: (sd[k].double().cpu() - torch.from_numpy(np.array(G["c_final_" + k])).double()).abs().max().item()
             for k in sd if sd[k].dtype.is_floating_point}
    d_param = max(diffs.values())
    print("largest state difference in", max(diffs, key=diffs.get))
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) / np.asarray(b) - 1).max())
    return d_param, rel(losses, G["c_losses"]), rel(norms, G["c_norms"])


def sequence_loader():
    """whole sequences as the evaluation loaders yield them: batches of one, the 2D side padded by the receptive field's half"""
    g = torch.Generator().manual_seed(91)
    pad = (MU.receptive_field(MU.SMALL["arch"]) - 1) // 2
    batches = []
    for T in (30, 41):
        b3 = 0.3 * torch.randn(1, T, 16, 3, generator=g)
        b2 = 0.4 * torch.randn(1, T, 16, 2, generator=g)
        b2 = torch.cat([b2[:, :1].expand(1, pad, 16, 2), b2, b2[:, -1:].expand(1, pad, 16, 2)], 1)
        batches.append((b3.cuda(), b2.cuda()))
    return batches


def test_video_loop_record_c_and_evaluation(D, G):
    """video_mode_train_posenet + posenet_optimizer with the strided class in 'bf16x6' on record (c)'s clips: final state, per-step
    losses and gradient norms within 4 x what stock torch gives on this GPU for the same loop.  Then video_mode_evaluate with the
    dilated class on whole sequences: its four metrics against the stock dilated module's with the same state."""
    cfg = MU.SMALL
    stock = make_stock(cfg)
    to_dev = [(a.cuda(), b.cuda()) for a, b in MU.train_batches()]
    s_losses, s_norms = PU.stock_loop(stock, "video", to_dev, torch.optim.Adam(stock.parameters(), lr=MU.TRAIN["lr"]),
                                      nn.MSELoss(reduction="mean"))
    d_stock = loop_diffs(stock, s_losses.cpu().numpy(), s_norms.cpu().numpy(), G)
    model = make(D, cfg, "bf16x6")
    D.V.video_mode_train_posenet(model, PU.loader_of("video", MU.train_batches()), D.T.posenet_optimizer(model, MU.TRAIN["lr"]),
                                 nn.MSELoss(reduction="mean"), torch.device("cuda"), PU.loop_args())
    trace = D.V.video_mode_train_posenet.last_trace.cpu().double().numpy()
    assert len(trace) == 12 == len(G["c_losses"])
    d_ours = loop_diffs(model, trace[:, 0], trace[:, 1], G)
    for name, s, o in zip(("param", "loss", "norm"), d_stock, d_ours):
        figure("c_stock_" + name, s), figure("c_ours_" + name, o)

    # evaluation: the trained state in both dilated modules
    args = argparse.Namespace(posenet_name="mulit_farme_videopose", architecture="3,3")
    ours_eval = make(D, cfg, "bf16x6", False, state={k: v.clone() for k, v in model.state_dict().items()})
    stock_eval = make_stock(cfg, False, state={k: v.clone() for k, v in model.state_dict().items()})
    batches = sequence_loader()
    m_ours = D.V.video_mode_evaluate(args, PU.EpochLoader(batches), ours_eval, torch.device("cuda"), get_pck_auc=True)
    m_stock = D.V.video_mode_evaluate(args, PU.EpochLoader(batches), stock_eval, torch.device("cuda"), get_pck_auc=True)
    # what 4 N of output error allows: every coordinate moves by at most e, a root-centred joint by at most d = 2 sqrt(3) e
    with torch.no_grad():
        outs = [stock_eval(b2) for _, b2 in batches]
    e = 4 * N_A["a8_"] * max(o.abs().max().item() for o in outs)
    d = 2 * math.sqrt(3.0) * e
    dist = torch.cat([((o - o[:, :, :1]) - (b3 - b3[:, :, :1])).norm(dim=-1).reshape(-1) for o, (b3, _) in zip(outs, batches)])
    thr = torch.tensor(D.loss.AUC_THRESHOLDS, device=dist.device, dtype=dist.dtype)
    near = ((1000 * dist.view(-1, 1) - thr.view(1, -1)).abs() <= 1000 * d).float().mean(0) * 100   # joints a threshold (mm) could count differently
    # (P-MPJPE fits a similarity transform first; its scale multiplies the moved distance.  Predictions and targets have the same
    # magnitude here, a scale beyond 4 would be a different network.)
    allow = (d * 1000, 4 * d * 1000, near[D.loss.PCK_INDEX].item(), near.mean().item())
    for name, a, b, lim in zip(("p1", "p2", "pck", "auc"), m_ours, m_stock, allow):
        print("FIGURE eval_%s ours %.6f stock %.6f allowed %.3g" % (name, a, b, lim))

    assert int(model.expand_bn.num_batches_tracked) == 12
    for name, s, o in zip(("param", "loss", "norm"), d_stock, d_ours):
        assert s <= 4 * N_LOOP[name], ("stock floor", name, s)
        assert o <= 4 * N_LOOP[name], (name, o)
    assert 0 < m_stock[2] < 100, "the evaluation data should put joints on both sides of the PCK threshold"
    for name, a, b, lim in zip(("p1", "p2", "pck", "auc"), m_ours, m_stock, allow):
        assert abs(a - b) <= lim + 1e-9 * abs(b), (name, a, b, lim)


@pytest.mark.parametrize("prec", ["bf16", "bf16x6"])
def test_optimizer_step_invalidates_packed_tap_operands(D, prec):
    """two PosenetAdam steps (the GEMMs read tap-major copies of the Conv1d weights cached on the parameters): the second step's
    forward equals, bit for bit, the forward of a freshly constructed module loaded with the stepped state"""
    cfg = MU.SMALL
    model = make(D, cfg, prec).train()
    opt = D.T.posenet_optimizer(model, 1e-2)
    x, t = MU.record_inputs(cfg, 8)
    x, t = x.cuda(), t.cuda()
    for step in range(2):
        state = {k: v.clone() for k, v in model.state_dict().items()}
        out, names = count_calls(D, lambda: model(x))
        packs = sum(1 for n in names if n in ("dhaug_conv_taps_pack_bf16", "dhaug_conv_taps_permute_f32"))
        assert packs == len(cfg["arch"]), names                   # each k-tap weight packed once per step, in the forward
        if step == 1:
            fresh = make(D, cfg, prec, state=state).train()
            assert torch.equal(out.detach(), fresh(x).detach()), "the forward after an optimizer step read stale tap operands"
        opt.zero_grad()
        nn.functional.mse_loss(out, t).backward()
        opt.clip_step(1)
    assert not torch.equal(model.state_dict()["layers_conv.0.weight"], state["layers_conv.0.weight"])
    # without a step in between nothing is packed again
    with torch.no_grad():
        model(x)
        _, names = count_calls(D, lambda: model(x))
    assert not [n for n in names if n in ("dhaug_conv_taps_pack_bf16", "dhaug_conv_taps_permute_f32")]


def bf16_emulation(cfg):
    """the stock network with what the 'bf16' mode rounds rounded: parameters (and, by the caller, inputs) to bf16, every convolution's
    and every activation's output to bf16 by forward hooks; the arithmetic itself stays fp32 on this GPU"""
    state = {k: (v.bfloat16().float() if v.dtype.is_floating_point and "running" not in k else v)
             for k, v in MU.seeded_state(cfg["C"], cfg["arch"], cfg["seed"]).items()}
    m = make_stock(cfg, state=state)
    rnd = lambda mod, inp, out: out.bfloat16().float()
    for mod in m.modules():
        if isinstance(mod, (nn.Conv1d, nn.ReLU)):
            mod.register_forward_hook(rnd)
    return m


def low_figures(m, G, cfg, B, prefix, round_input=False):
    x, t = MU.record_inputs(cfg, B)
    x, t = x.cuda(), t.cuda()
    if round_input:
        x = x.bfloat16().float()
    m.train()
    out = m(x)
    loss = nn.functional.mse_loss(out, t)
    loss.backward()
    ref = lambda n: torch.from_numpy(np.array(G[prefix + n]))
    fig = dict(out=(out.detach().double().cpu() - ref("out")).abs().max().item() / ref("out").abs().max().item(),
               loss=abs(loss.item() / ref("loss").item() - 1), grad=0.0)
    for k, p in m.named_parameters():
        r = ref("grad_" + k)
        fig["grad"] = max(fig["grad"], ((p.grad.double().cpu() - r).norm() / r.norm()).item())
    return fig


def test_throughput_modes_against_the_bf16_emulation(D, G):
    """'bf16': output, loss and the worst relative L2 of a gradient tensor, each against the fp64 record a8, within 4 x the same
    figure of the bf16 emulation of the stock network; 'bf16x3' lies between 'bf16' and 'bf16x6' and is held to the 'bf16' bound.
    Neither is a parity mode."""
    cfg, B, prefix = MU.SMALL, 8, "a8_"
    emu = low_figures(bf16_emulation(cfg), G, cfg, B, prefix, round_input=True)
    figs = {prec: low_figures(make(D, cfg, prec), G, cfg, B, prefix) for prec in ("bf16", "bf16x3")}
    for k in ("out", "loss", "grad"):
        figure("emulation_" + k, emu[k]), figure("bf16_" + k, figs["bf16"][k]), figure("bf16x3_" + k, figs["bf16x3"][k])
    for prec in ("bf16", "bf16x3"):
        for k in ("out", "loss", "grad"):
            assert figs[prec][k] <= 4 * emu[k], (prec, k, figs[prec][k], emu[k])


def test_dropout_follows_the_device_generator(D):
    """torch.manual_seed reproduces a training forward with dropout; consecutive calls draw different masks"""
    model = make(D, MU.SMALL, "bf16x6", dropout=0.25).train()
    x = MU.record_inputs(MU.SMALL, 8)[0].cuda()
    with torch.no_grad():
        torch.manual_seed(5)
        a, a2 = model(x), model(x)
        torch.manual_seed(5)
        b = model(x)
        torch.manual_seed(6)
        c = model(x)
    assert torch.equal(a, b) and not torch.equal(a, a2) and not torch.equal(a, c)


def test_training_shape_errors(D):
    m = make(D, MU.SMALL, "bf16x6").train()
    with pytest.raises(ValueError, match="one receptive field"):
        m(torch.zeros(4, 12, 16, 2, device="cuda"))
    one = make(D, dict(C=32, arch=(3,), seed=1), "bf16x6").train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        one(torch.zeros(1, 3, 16, 2, device="cuda"))
    assert one(torch.zeros(2, 3, 16, 2, device="cuda")).shape == (2, 1, 16, 3)
