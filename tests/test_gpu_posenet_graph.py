"""GPU tests of the replayed posenet training step (StepRunner(graph=True), function_aug/model_pos_train.py) on small models.

Each run is three epochs (one StepRunner each, as the loops build them) of three full batches and one ragged batch, from one seed and
one initial state: the full batch's step is captured at its third sighting (epoch 1), the ragged batch's in epoch 3.

The yardstick of "equal to the eager path" is the eager path itself: the weight-gradient GEMMs add split-K partials with fp32 atomics,
so two graph=False runs of one loop need not agree bit for bit.  Per tensor, D = the largest absolute difference between two
graph=False runs; where D is 0 the graph run must equal the eager run bit for bit, elsewhere it may differ by at most 4 D (the
project's convention).  Every comparison prints its figures ("FIGURE ...") before it asserts.  Counters (steps, poses,
num_batches_tracked) are compared exactly."""
import argparse
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import gcn_util as CU
import poseformer_util as FU
import posenet_util as NU
import video_posedata_util as VU

pytestmark = pytest.mark.gpu

LR = 1e-3
EPOCHS = 3
P_DROP = 0.25


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dhaug_amd import autograd_ops, ops, optim
    from dhaug_amd.function_aug import model_pos_train
    from dhaug_amd.models_baseline.gcn.sem_gcn import SemGCN
    from dhaug_amd.models_baseline.mlp.linear_model import LinearModel
    from dhaug_amd.models_baseline.poseformer.model_poseformer import PoseTransformer
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    from dhaug_amd.models_Fk_GAN import model_fk_gan_train, video_mode_operate
    from dhaug_amd.models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModelOptimized1f
    from dhaug_amd.utils.loss import mpjpe
    return argparse.Namespace(A=autograd_ops, ops=ops, optim=optim, T=model_pos_train, V=video_mode_operate, train=model_fk_gan_train,
                              SemGCN=SemGCN, LinearModel=LinearModel, PoseTransformer=PoseTransformer,
                              Single=TemporalModelOptimized1f, Multi=multiFrame_TemporalModelOptimized1f, mpjpe=mpjpe)


# ---------------------------------------------------------------------------------------------------------------- the small models
def build(M, name):
    torch.manual_seed(17)
    if name == "videopose":
        cfg = NU.SMALL
        return M.Single(16, 2, 15, [1] * (cfg["stages"] + 1), dropout=P_DROP, channels=cfg["C"])
    if name == "mlp":
        return M.LinearModel(32, 45, linear_size=64, num_stage=2, p_dropout=P_DROP)
    if name == "mulit_farme_videopose":
        return M.Multi(16, 2, 16, [3], dropout=P_DROP, channels=32)
    assert name == "gcn"
    return M.SemGCN(CU.adj_matrix(), 32, num_layers=2, p_dropout=P_DROP)


def batches_of(name):
    """three full batches and a ragged one, on the device: [(inputs, targets)]"""
    g = torch.Generator().manual_seed(23)
    sizes = {"videopose": (24, 9), "mlp": (24, 9), "mulit_farme_videopose": (6, 2), "gcn": (6, 4)}[name]
    out = []
    for n in (sizes[0],) * 3 + (sizes[1],):
        if name == "mulit_farme_videopose":
            x, t = torch.randn(n, 3, 16, 2, generator=g) * 0.4, torch.randn(n, 1, 16, 3, generator=g)
        else:
            x, t = torch.randn(n, 16, 2, generator=g) * 0.4, torch.randn(n, 16, 3, generator=g)
        t = t - t[..., :1, :]
        out.append((x.cuda(), t.cuda()))
    return out


def set_dropout(model, p):
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = p


def generator():
    return torch.cuda.default_generators[torch.cuda.current_device()]


class Run:
    """a model, its optimizer and the epochs run on it so far"""

    def __init__(self, M, name, prec, crit, graph):
        self.M, self.name, self.graph = M, name, graph
        self.model = build(M, name).cuda().train()
        self.model.precision = prec
        self.opt = M.T.posenet_optimizer(self.model, LR)
        self.criterion = nn.MSELoss(reduction="mean") if crit == "mse" else M.mpjpe
        self.batches = batches_of(name)
        self.traces, self.meters, self.runners = [], [], []
        torch.manual_seed(5)                       # the device generator: seed 5, offset 0

    def epoch(self, batches=None):
        r = self.M.T.StepRunner(self.model, self.opt, self.criterion, torch.device("cuda"), graph=self.graph)
        for x, t in (self.batches if batches is None else batches):
            r.step(x, t, "loss", x.shape[0])
        self.meters.append(r.finish(False))
        self.traces.append(r.trace_tensor().clone())
        self.runners.append(r)
        return r

    def state(self):
        """every tensor the comparison looks at, on the host"""
        torch.cuda.synchronize()
        s = {"param " + k: v.detach() for k, v in self.model.named_parameters()}
        s.update({"buffer " + k: v for k, v in self.model.named_buffers()})
        s.update({"exp_avg": self.opt.exp_avg, "exp_avg_sq": self.opt.exp_avg_sq, "step_dev": self.opt.step_dev})
        s.update({"trace %d" % e: t for e, t in enumerate(self.traces)})
        return {k: v.cpu().clone() for k, v in s.items()}


_RUNS = {}


def three_runs(M, name, prec, crit):
    """(eager, eager again, graph) after EPOCHS epochs, with the generator offset each run ended on; computed once per configuration"""
    key = (name, prec, crit)
    if key not in _RUNS:
        out = []
        for graph in (False, False, True):
            r = Run(M, name, prec, crit, graph)
            for _ in range(EPOCHS):
                r.epoch()
            out.append((r, r.state(), generator().get_offset()))
        _RUNS[key] = out
    return _RUNS[key]


CONFIGS = [(n, p, "mse") for n in ("videopose", "mlp", "mulit_farme_videopose", "gcn") for p in ("bf16", "bf16x6")] + \
          [("mulit_farme_videopose", p, "mpjpe") for p in ("bf16", "bf16x6")]


# --------------------------------------------------------------------------------------------------- 1. equal to the eager path
@pytest.mark.parametrize("name,prec,crit", CONFIGS)
def test_graph_run_equals_the_eager_run(M, name, prec, crit):
    """Measured (MI355X, gfx950, 2026-10-20, two runs of this file): in all ten configurations two graph=False runs agree bit for bit
    in every tensor, and so does the graph run.  gcn-bf16x6 used not to: its weight-gradient GEMM contracts 6 x 96 rows, which
    dhaug_gemm_tn_bf16_rows cut in three slices that add with atomics (eager-eager distances up to 4.1e-03, and a tensor that moved
    by one ulp missed the rule below by chance in seven of eight runs).  A contraction of fewer than 1 024 rows is now cut in at most
    two slices, whose sum onto a zeroed output does not depend on their order."""
    (ea, sa, _), (eb, sb, _), (gr, sg, _) = three_runs(M, name, prec, crit)
    assert set(sa) == set(sb) == set(sg)
    worst = 0.0
    bad = []
    for k in sorted(sa):
        a, b, g = sa[k], sb[k], sg[k]
        if not a.dtype.is_floating_point:                         # num_batches_tracked, the device step count
            assert torch.equal(a, g) and torch.equal(a, b), k
            continue
        assert torch.isfinite(g).all(), k
        D = (a.double() - b.double()).abs().max().item()
        d = (a.double() - g.double()).abs().max().item()
        worst = max(worst, D)
        if D == 0.0:
            if not torch.equal(a.view(torch.int32), g.view(torch.int32)):
                bad.append((k, D, d))
        elif d > 4 * D:
            bad.append((k, D, d))
        if d > 0 or D > 0:
            print("FIGURE %s %s %s %s: eager-eager %.3e graph-eager %.3e" % (name, prec, crit, k, D, d))
    print("FIGURE %s %s %s: largest eager-eager distance of any tensor %.3e" % (name, prec, crit, worst))
    assert not bad, bad
    assert int(sg["step_dev"]) == 4 * EPOCHS == gr.opt.step_count == ea.opt.step_count
    for e in range(EPOCHS):
        ma, mb, mg = ea.meters[e], eb.meters[e], gr.meters[e]
        for k in ma:
            if k.endswith("_poses") or k.endswith("_steps") or k == "steps":
                assert ma[k] == mg[k], (e, k)
            else:
                D = abs(ma[k] - mb[k])
                assert (mg[k] == ma[k]) if D == 0 else (abs(mg[k] - ma[k]) <= 4 * D), (e, k, ma[k], mg[k], D)
        assert mg["loss_steps"] == 4 and mg["loss_poses"] == sum(x.shape[0] for x, _ in gr.batches)
    # the training moved something (the comparison above is not between two untouched models)
    fresh = build(M, name).state_dict()
    assert any(not torch.equal(sg["param " + k], v) for k, v in fresh.items() if "param " + k in sg)


# -------------------------------------------------------------------------------------------------------------------- 2. masks
@pytest.mark.parametrize("name,prec,crit", CONFIGS)
def test_generator_and_rng_cell_end_where_the_eager_run_ends(M, name, prec, crit):
    (ea, _, off_a), (eb, _, off_b), (gr, _, off_g) = three_runs(M, name, prec, crit)
    st = gr.opt._dhaug_graph_state
    steps = 4 * EPOCHS
    K = st.dropout.calls // steps                                 # dropout calls per step: the hidden BatchNorm layers
    assert K >= 1 and st.dropout.calls == K * steps
    assert off_a == off_b == 4 * K * steps                        # what the eager path's host-side stream arrives at
    assert off_g == off_a
    cell = st.rng_cell.cpu().tolist()
    assert cell[0] == 5                                           # the seed of torch.manual_seed(5)
    # the last epoch's stream started where the generator stood (4 K steps of two epochs) and has moved by 4 K per step since
    assert cell[1] == 4 * K * 4 * (EPOCHS - 1) + 4 * K * 4 == off_g


def test_replays_draw_new_masks(M):
    """lr = 0: the weights stand still, so two replays on identical inputs differ by their masks alone -- different losses at
    p = 0.25, and at p = 0 (a key of its own: two warm-up steps and a capture) bit-equal ones"""
    r = Run(M, "videopose", "bf16x6", "mse", True)
    x, t = r.batches[0]
    r.epoch([(x, t)] * 3)                                         # two eager steps, capture + replay
    assert r.runners[-1].replayed_steps == 1
    r.opt.param_groups[0]["lr"] = 0.0
    before = r.opt.flat_param.clone()
    run = r.epoch([(x, t)] * 3)
    assert run.replayed_steps == 3 and run.eager_steps == 0
    loss = r.traces[-1][:, 0].cpu()
    assert loss[0] != loss[1] and loss[1] != loss[2] and torch.isfinite(loss).all()
    assert torch.equal(r.opt.flat_param, before)
    set_dropout(r.model, 0.0)
    run = r.epoch([(x, t)] * 5)                                   # p = 0: eager, eager, capture + replay, replay, replay
    assert (run.eager_steps, run.replayed_steps, run.captures) == (2, 3, 2)
    tr = r.traces[-1].cpu()
    assert torch.equal(tr[2], tr[3]) and torch.equal(tr[3], tr[4]) and torch.equal(tr[0], tr[2])
    assert torch.equal(r.opt.flat_param, before)
    assert r.opt._dhaug_graph_state.dropout.calls == 6 * 5        # p = 0 draws nothing: the count stands where p = 0.25 left it


# ---------------------------------------------------------------------------------------------------------- 3. replays happen
@pytest.mark.parametrize("name,prec,crit", [CONFIGS[0], CONFIGS[3], CONFIGS[5], CONFIGS[6], CONFIGS[9]])
def test_counters_follow_the_schedule(M, name, prec, crit):
    (ea, _, _), _, (gr, _, _) = three_runs(M, name, prec, crit)
    # epoch 1: full batch eager, eager, capture + replay; ragged eager.  Epoch 2: three replays; ragged eager.  Epoch 3: three
    # replays; the ragged batch's third sighting: capture + replay
    assert [(r.eager_steps, r.replayed_steps) for r in gr.runners] == [(3, 1), (1, 3), (0, 4)]
    assert [(r.eager_steps, r.replayed_steps, r.captures) for r in ea.runners] == [(4, 0, 0)] * EPOCHS
    st = gr.opt._dhaug_graph_state
    assert st.captures == 2 == gr.runners[-1].captures and len(st.steps) == 2
    assert not hasattr(ea.opt, "_dhaug_graph_state")


def test_second_runner_replays_from_its_first_step(M):
    gr = three_runs(M, "videopose", "bf16", "mse")[2][0]
    r = gr.epoch()                                                # a fourth epoch: a new StepRunner on the same optimizer
    assert (r.eager_steps, r.replayed_steps, r.captures) == (0, 4, 2)
    assert gr.meters[-1]["loss_steps"] == 4 and np.isfinite(gr.meters[-1]["loss"])
    assert gr.opt.step_count == 4 * (EPOCHS + 1) == int(gr.opt.step_dev.item())
    del _RUNS[("videopose", "bf16", "mse")]                       # (this run has moved on: later tests build their own)


@pytest.mark.parametrize("name,prec", [("videopose", "bf16"), ("mulit_farme_videopose", "bf16x6"), ("gcn", "bf16")])
def test_replays_survive_a_cache_release(M, name, prec):
    """The captured steps hold addresses.  After torch.cuda.empty_cache() (every later capture calls it) and after the memory the
    allocator had cached has been handed out, filled with NaN and freed again, further epochs of replays still equal the eager
    path bit for bit (these configurations repeat their bits).  Found with this test's scenario: with the library's own memsets in the
    graph the most recently captured step returned gradient norms of 1e23 .. 1e30 after the release; see ops.ZERO_BY_KERNEL."""
    out = {}
    for graph in (False, True):
        r = Run(M, name, prec, "mse", graph)
        for _ in range(EPOCHS):
            r.epoch()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        r.epoch()
        keep = [torch.full((size // 4,), float("nan"), device="cuda") for size in (512, 4096, 32768, 262144, 1 << 21) for _ in range(16)]
        torch.cuda.synchronize()
        del keep
        run = r.epoch()
        assert (run.eager_steps, run.replayed_steps) == ((0, 4) if graph else (4, 0))
        out[graph] = (torch.cat(r.traces[EPOCHS:]).cpu(), r.opt.flat_param.cpu().clone())
    assert torch.isfinite(out[True][0]).all()
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])


# --------------------------------------------------------------------------------------------------------------------- 4. lr
def test_changed_lr_takes_effect_at_the_next_replay(M):
    runs = []
    for lr in (LR, 10 * LR):
        r = Run(M, "mlp", "bf16x6", "mse", True)
        x, t = r.batches[0]
        r.epoch([(x, t)] * 4)
        r.opt.param_groups[0]["lr"] = lr
        run = r.epoch([(x, t)] * 2)
        assert (run.eager_steps, run.replayed_steps) == (0, 2)
        runs.append(r.opt.flat_param.clone())
    # the same seed, state and masks: the two runs differ by the learning rate of their last two replays alone
    assert not torch.equal(runs[0], runs[1])
    assert (runs[0] - runs[1]).abs().max().item() > 1e-3
    r.opt.param_groups[0]["lr"] = 0.0
    before, m_before = r.opt.flat_param.clone(), r.opt.exp_avg.clone()
    run = r.epoch([(x, t)] * 3)
    assert run.replayed_steps == 3
    assert torch.equal(r.opt.flat_param.view(torch.int32), before.view(torch.int32))
    assert not torch.equal(r.opt.exp_avg, m_before)


# ----------------------------------------------------------------------------------------------------------------- 5. caches
@pytest.mark.parametrize("name", ["videopose", "mlp", "mulit_farme_videopose", "gcn"])
def test_evaluation_after_replays_sees_the_new_weights(M, name):
    """the analogue of test_optimizer_step_invalidates_packed_weights: a replay writes parameters and running statistics through raw
    pointers, and the host bookkeeping behind it must make every cached operand and every folded evaluation layer stale"""
    r = Run(M, name, "bf16", "mse", True)
    x, t = r.batches[0]

    def evaluate(model):
        model.eval()
        with torch.no_grad():
            return model(x).clone()

    y0 = evaluate(r.model)                                        # builds the evaluation cache of the initial weights
    r.model.train()
    run = r.epoch([(x, t)] * 4)
    assert run.replayed_steps == 2
    y1 = evaluate(r.model)                                        # ... and of the weights after two eager steps and two replays
    r.model.train()
    run = r.epoch([(x, t)] * 2)
    assert (run.eager_steps, run.replayed_steps) == (0, 2)       # nothing but replays since y1
    y2 = evaluate(r.model)
    fresh = build(M, name).cuda()
    fresh.precision = "bf16"
    fresh.load_state_dict(r.model.state_dict())
    yf = evaluate(fresh)
    assert not torch.equal(y0, y2) and not torch.equal(y1, y2)
    assert torch.equal(y2.view(torch.int32), yf.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- 6. the three loops
def loop_args(playback):
    return argparse.Namespace(flip_pos_model_input=True, GAN_video_playback_input=playback, posenet_graph=True)


def check_loop(fn, steps, poses, flip_only):
    m, tr = fn.last_meters, fn.last_trace
    assert m is not None and m["steps"] == steps and tuple(tr.shape) == (steps, 2)
    assert torch.isfinite(tr).all() and (tr > 0).all()
    assert m["loss_poses"] == poses and np.isfinite(m["loss"]) and m["loss"] > 0
    assert m["flip_loss"] == m["loss"] and m["flip_loss_poses"] == m["loss_poses"] and m["flip_loss_steps"] == m["loss_steps"]
    if not flip_only:
        assert m["back_loss_poses"] == poses and m["back_flip_loss_poses"] == poses and np.isfinite(m["back_flip_loss"])


def test_train_posenet_on_a_fake_pair_buffer(M):
    g = torch.Generator().manual_seed(3)
    buf = M.train.FakePairBuffer(8)
    buf.append((torch.randn(20, 16, 3, generator=g)).cuda(), (torch.randn(20, 16, 2, generator=g) * 0.4).cuda(), [0.0] * 9)
    model = build(M, "videopose").cuda()
    opt = M.T.posenet_optimizer(model, LR)
    torch.manual_seed(7)
    for epoch in range(3):                                        # 8 + 8 + 4 pairs, plain and flipped: 6 steps per epoch
        M.T.train_posenet(model, buf, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"), loop_args(False))
        check_loop(M.T.train_posenet, 6, 20, True)
    st = opt._dhaug_graph_state
    # four keys (full / ragged x plain / flipped); the full ones are seen twice per epoch: captured in epoch 2, the ragged in 3
    assert st.captures == 4 and opt.step_count == 18 == int(opt.step_dev.item())
    # the permutation of an epoch and the dropout masks share the generator: it ends past both
    assert generator().get_offset() >= 4 * st.dropout.calls > 0


def video_model(M):
    return build(M, "mulit_farme_videopose").cuda()


def test_gan_dataset_video_loop_on_a_fake_pair_buffer(M):
    g = torch.Generator().manual_seed(4)
    buf = M.train.FakePairBuffer(8)
    buf.append(torch.randn(20, 1, 16, 3, generator=g).cuda(), (torch.randn(20, 3, 16, 2, generator=g) * 0.4).cuda(), [0.0] * 9)
    model = video_model(M)
    opt = M.T.posenet_optimizer(model, LR)
    fn = M.V.GAN_dataSet_video_mode_train_posenet
    for epoch in range(3):                                        # 3 batches x (plain, playback, flip, flip + playback)
        fn(model, buf, opt, M.mpjpe, torch.device("cuda"), loop_args(True))
        check_loop(fn, 12, 20, False)
    assert opt._dhaug_graph_state.captures == 8 and opt.step_count == 36


def test_video_loop_on_a_chunked_generator(M):
    rng = np.random.RandomState(6)
    lengths = (11, 9)
    p3 = [rng.randn(n, 16, 3).astype(np.float32) for n in lengths]
    p2 = [(rng.randn(n, 16, 2) * 0.4).astype(np.float32) for n in lengths]
    cam = [rng.randn(16).astype(np.float32) for _ in lengths]
    loader = M.V.ChunkedGenerator(8, cam, p3, p2, chunk_length=1, pad=1, **VU.LR)
    model = video_model(M)
    opt = M.T.posenet_optimizer(model, LR)
    fn = M.V.video_mode_train_posenet
    for epoch in range(3):                                        # 20 clips of 3 frames: 8 + 8 + 4
        fn(model, loader, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"), loop_args(False))
        check_loop(fn, 6, 20, True)
    assert opt._dhaug_graph_state.captures == 4 and opt.step_count == 18


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_come_before_any_capture(M):
    dev = torch.device("cuda")
    mse = nn.MSELoss(reduction="mean")
    model = build(M, "videopose").cuda().train()
    opt = M.T.posenet_optimizer(model, LR)
    with pytest.raises(ValueError, match="clip_step"):
        M.T.StepRunner(model, torch.optim.Adam(build(M, "videopose").cuda().parameters()), mse, dev, graph=True)
    for crit in (nn.L1Loss(), nn.MSELoss(reduction="sum"), lambda a, b: (a - b).abs().mean()):
        with pytest.raises(ValueError, match="fused criteria"):
            M.T.StepRunner(model, opt, crit, dev, graph=True)
    opt.world_size = lambda: 2
    with pytest.raises(NotImplementedError, match="world size"):
        M.T.StepRunner(model, opt, mse, dev, graph=True)
    del opt.world_size
    former = M.PoseTransformer(**FU.kwargs(FU.LOOP)).cuda().train()
    with pytest.raises(NotImplementedError, match="PoseTransformer"):
        M.T.StepRunner(former, M.T.posenet_optimizer(former, LR), mse, dev, graph=True)
    stub = nn.Linear(32, 48).cuda()
    with pytest.raises(NotImplementedError, match="supports"):
        M.T.StepRunner(stub, M.T.posenet_optimizer(stub, LR), mse, dev, graph=True)
    assert not hasattr(opt, "_dhaug_graph_state")                 # none of them got as far as the graph state
    run = M.T.StepRunner(model, opt, mse, dev, graph=True)
    model.eval()
    x, t = batches_of("videopose")[0]
    with pytest.raises(RuntimeError, match="training mode"):
        run.step(x, t, "loss", x.shape[0])
    assert run.steps == 0 and run.captures == 0 and not opt._dhaug_graph_state.steps
    assert not torch.cuda.is_current_stream_capturing() and M.A.CAPTURE_ID == 0 and M.A.DEVICE_DROPOUT is None
    # the same objects without graph=True are accepted as before
    M.T.StepRunner(model, torch.optim.Adam(model.parameters()), nn.L1Loss(), dev)


def test_no_capture_warning_on_the_supported_models(M):
    """a capture that raises is survived with a warning and an eager key; on the supported models none may be needed"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = Run(M, "gcn", "bf16x6", "mse", True)
        x, t = r.batches[0]
        run = r.epoch([(x, t)] * 3)
    assert (run.eager_steps, run.replayed_steps, run.captures) == (2, 1, 1)
