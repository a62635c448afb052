"""n_mpjpe, weighted_mpjpe, mpjpe_byjoint and JointWeightedMpjpe of utils.loss as training criteria on the GPU: against torch's
autograd of the reference's expressions and against the reference's own gradients (tests/golden/pose_criteria.npz, group a), the
two video loops end to end with the two fused ones against group (b), the host reads of a fused epoch, and
StepRunner(graph=True) with them."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import pose_criteria_util as CU
import posetrain_mpjpe_util as MU
import posetrain_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# the project's convention for the end-to-end comparison (tests/test_gpu_posetrain_mpjpe.py): N = what the stock-torch run of the
# same loop on this device is away from the CPU-recorded fixture, measured in the test; the drop-in is held to
# 4 * max(N, SAME_DEVICE_FLOOR) against the fixture
SAME_DEVICE_FLOOR = 2.69e-6
CHAOS_LIMIT = 1e-3


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    from dhaug_amd import _lib, ops
    from dhaug_amd.function_aug import model_pos_train
    from dhaug_amd.models_Fk_GAN import video_mode_operate
    from dhaug_amd.utils import loss
    fns = dict(video=video_mode_operate.video_mode_train_posenet, gan=video_mode_operate.GAN_dataSet_video_mode_train_posenet)
    return argparse.Namespace(lib=_lib, ops=ops, T=model_pos_train, V=video_mode_operate, fns=fns, loss=loss)


@pytest.fixture(scope="module")
def G():
    return CU.load_golden()


@pytest.fixture(scope="module")
def clips():
    return MU.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def node(v):
    return type(v.grad_fn).__name__


def on_kernels(v):
    return v.grad_fn is not None and ("_ScalarCriterionFn" in node(v) or "_ByJointFn" in node(v))


# --------------------------------------------------------------------------------------------------- the three functions
@pytest.mark.parametrize("k", range(len(CU.SHAPES)))
def test_criteria_against_torch_autograd_and_the_reference(M, G, k):
    """value and gradient of the three functions on an fp32 device prediction that requires grad.  Against torch's autograd of the
    reference's expressions on this device: rtol = 1e-6 with no absolute term, as the mpjpe test -- evaluated in fp64 there, because
    the N-MPJPE gradient is a difference of two terms and an fp32 evaluation of the EXPRESSION misses 1e-6 of a small element by
    its own rounding.  Against the reference's own fp64 gradients (the fixture): the bounds of pose_criteria_util plus the
    fixture's own roundoff (1e-12 of its largest element)."""
    L = M.loss
    g = lambda name: G["a%d_%s" % (k, name)]
    shape = CU.SHAPES[k]
    x, y64, x64 = dev(g("target")), dev(g("pred")).double(), dev(g("target")).double()
    cot = dev(g("cot"))
    poses = int(np.prod(shape[:-2]))
    _, _, T = CU.nmpjpe(g("pred"), g("target"))
    w = {c: dev(g(name)) for c, name in (("wp", "w_pose"), ("wj", "w_joint"))}
    w["w16"] = dev(g("w16")).expand(shape[:-1])
    calls = dict(n=(lambda p: L.n_mpjpe(p, x), lambda p: CU.torch_n_mpjpe(p, x64)),
                 bj=(lambda p: L.mpjpe_byjoint(p, x), lambda p: CU.torch_mpjpe_byjoint(p, x64)))
    for c in w:
        calls[c] = (lambda p, c=c: L.weighted_mpjpe(p, x, w[c]), lambda p, c=c: CU.torch_weighted_mpjpe(p, x64, w[c].double()))
    for c, (ours, theirs) in calls.items():
        p = dev(g("pred")).requires_grad_(True)
        v = ours(p)
        assert on_kernels(v) and v.is_cuda and v.dtype == torch.float32, c
        p64 = y64.clone().requires_grad_(True)
        r = theirs(p64)
        if c == "bj":
            assert tuple(v.shape) == shape[1:-1]
            (v * cot).sum().backward()
            (r * cot.double()).sum().backward()
        else:
            assert v.dim() == 0
            v.backward()
            r.backward()
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32
        assert torch.allclose(p.grad.double(), p64.grad, rtol=1e-6, atol=0), c
        assert torch.allclose(v.detach().double(), r.detach(), rtol=1e-6, atol=0), c
        # the fixture
        got, want = p.grad.cpu().double().numpy(), g(c + "_grad")
        bound = CU.nmpjpe_bound(want, T, poses) if c == "n" else CU.ulp32(want)
        err = np.abs(got - want)
        print("criterion %s case %d: gradient at %.3f of its bound against the reference" % (c, k, float((err / bound).max())))
        assert (err <= bound + 1e-12 * np.abs(want).max()).all(), c
        val, vwant = v.detach().cpu().double().numpy(), g(c + "_value")
        assert (np.abs(val - vwant) <= CU.ulp32(vwant) + 1e-12 * np.abs(vwant).max()).all(), c
        if c == "bj":                                             # the differentiable value IS the metric's value
            assert torch.equal(v.detach(), L.mpjpe_byjoint(p.detach(), x))
        with torch.no_grad():                                     # gradients off: the metric, as before
            off = ours(p)
        assert off.grad_fn is None and torch.equal(off, ours(p.detach()))


def test_every_other_call_keeps_the_torch_expression(M, G):
    """the fall-backs: fp64, a target or w that requires grad, more than COLERR_MAX_COLS joints per entry and the one-pose form of
    mpjpe_byjoint keep a grad_fn from the plain torch expression; host inputs stay on the host"""
    L = M.loss
    y, x, wp = dev(G["a1_pred"]), dev(G["a1_target"]), dev(G["a1_w_pose"])
    p = y.clone().requires_grad_(True)
    cases = [L.n_mpjpe(p.double(), x.double()), L.weighted_mpjpe(p.double(), x.double(), wp.double()),
             L.mpjpe_byjoint(p.double(), x.double()),                                            # fp64
             L.n_mpjpe(p, x.clone().requires_grad_(True)), L.weighted_mpjpe(p, x.clone().requires_grad_(True), wp),
             L.mpjpe_byjoint(p, x.clone().requires_grad_(True)),                                 # the target asks for a gradient
             L.weighted_mpjpe(p, x, wp.clone().requires_grad_(True)),                            # the weights do
             L.mpjpe_byjoint(p[0, 0], x[0, 0])]                                                  # one pose
    wide = M.lib.COLERR_MAX_COLS // 16 + 1
    big = torch.randn(2, wide, 16, 3, device="cuda")
    cases.append(L.mpjpe_byjoint(big.clone().requires_grad_(True), big + 1))
    for i, v in enumerate(cases):
        assert v.grad_fn is not None and not on_kernels(v), (i, node(v))
    assert cases[0].dtype == torch.float64 and cases[-2].dim() == 0 and tuple(cases[-1].shape) == (wide, 16)
    t = x.clone().requires_grad_(True)
    L.n_mpjpe(p, t).backward()
    assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().sum()) > 0
    # values: the torch expression is the reference's
    assert torch.allclose(cases[3], CU.torch_n_mpjpe(p, x), rtol=1e-6) and torch.allclose(cases[6], CU.torch_weighted_mpjpe(p, x, wp))
    hp = y.cpu().requires_grad_(True)
    for v in (L.n_mpjpe(hp, x.cpu()), L.weighted_mpjpe(hp, x.cpu(), wp.cpu()), L.mpjpe_byjoint(hp, x.cpu())):
        assert not v.is_cuda and v.grad_fn is not None and not on_kernels(v)
    with pytest.raises(ValueError, match="B, F, 16, 3"):
        L.n_mpjpe(p[0], x[0])


def test_joint_weighted_mpjpe_equals_weighted_mpjpe(M, G):
    """JointWeightedMpjpe against weighted_mpjpe with the sixteen weights expanded over every pose: bit for bit, in loss and
    gradient (the shared-weight kernel reads what the per-joint one reads); host inputs and gradient-free calls as weighted_mpjpe
    evaluates them"""
    L = M.loss
    for k, shape in enumerate(CU.SHAPES):
        y, x, w16 = dev(G["a%d_pred" % k]), dev(G["a%d_target" % k]), G["a%d_w16" % k]
        crit = L.JointWeightedMpjpe(w16)
        p1, p2 = y.clone().requires_grad_(True), y.clone().requires_grad_(True)
        v1, v2 = crit(p1, x), L.weighted_mpjpe(p2, x, dev(w16).expand(shape[:-1]))
        assert on_kernels(v1) and on_kernels(v2) and v1.dim() == 0
        (2 * v1).backward()
        (2 * v2).backward()
        assert torch.equal(v1, v2) and torch.equal(p1.grad, p2.grad) and float(p1.grad.abs().sum()) > 0
        assert crit.weights.is_cuda and crit.buffer(y.device) is crit.weights
        plain = crit(y, x)
        assert plain.grad_fn is None and torch.equal(plain, L.weighted_mpjpe(y, x, dev(w16).expand(shape[:-1])))
        host = L.JointWeightedMpjpe(w16)(G["a%d_pred" % k], G["a%d_target" % k])
        want = L.weighted_mpjpe(G["a%d_pred" % k], G["a%d_target" % k], torch.from_numpy(w16).expand(shape[:-1]))
        assert not host.is_cuda and torch.equal(host, want) and torch.equal(host, plain.cpu())
        p64 = y.double().requires_grad_(True)
        v64 = crit(p64, x.double())
        assert v64.dtype == torch.float64 and v64.grad_fn is not None and not on_kernels(v64)


# ------------------------------------------------------------------------------------------------------------ end to end
def _criteria(M):
    """criterion name -> (the drop-in's criterion, the stock-torch callable)"""
    w16 = dev(CU.LOOP_W16)
    return dict(n=(M.loss.n_mpjpe, CU.torch_n_mpjpe),
                w16=(M.loss.JointWeightedMpjpe(CU.LOOP_W16), lambda p, t: CU.torch_weighted_mpjpe(p, t, w16.expand(p.shape[:-1]))))


def _run_drop_in(M, V, loop, criterion, numpy_batches=False):
    model = PU.load_initial(MU.make_model(loop), V, loop).cuda()
    opt = M.T.posenet_optimizer(model, PU.LR)
    if numpy_batches:                                             # what the reference's ChunkedGenerator yields
        batches = [(b3.double().numpy(), b2.double().numpy()) for b3, b2 in PU.batches_of(V, loop)]
    else:
        batches = PU.batches_of(V, loop, dev if loop == "video" else (lambda a: torch.from_numpy(np.ascontiguousarray(a))))
    fn = M.fns[loop]
    fn(model, PU.loader_of(loop, batches), opt, criterion, torch.device("cuda"), PU.loop_args())
    trace = fn.last_trace.cpu().double().numpy()
    return model, trace[:, 0], trace[:, 1], fn.last_meters


def _rel(a, b):
    return float(np.abs(np.asarray(a) / np.asarray(b) - 1).max())


def _state_diff(a, b):
    sa, sb = PU.state_arrays(a), PU.state_arrays(b)
    return max(float(np.abs(sa[k] - sb[k]).max()) for k in sa)


@pytest.mark.parametrize("c", CU.CRITERIA)
@pytest.mark.parametrize("loop", CU.LOOPS)
def test_video_loops_end_to_end(M, G, clips, loop, c):
    """video_mode_train_posenet / GAN_dataSet_video_mode_train_posenet with n_mpjpe and with JointWeightedMpjpe, PosenetAdam, flip
    and playback on, against the reference's run of the same loop (fixture group b): final parameters, BatchNorm buffers (absolute),
    per-step losses and norms (relative) within 4 * max(N, SAME_DEVICE_FLOOR), N being what stock torch on this device is away
    from the fixture.  (Before these were fused criteria the loops ran them on the generic path; with graph=True: ValueError.)
    Measured on an MI355X: see the README's bullet on the criteria."""
    V = CU.loop_view(G, clips, c, loop)
    ours, stock_crit = _criteria(M)[c]
    stock = PU.load_initial(MU.make_model(loop), V, loop).cuda()
    s_losses, s_norms = PU.stock_loop(stock, loop, PU.batches_of(V, loop, dev), torch.optim.Adam(stock.parameters(), lr=PU.LR),
                                      stock_crit)
    N = (PU.max_state_diff(stock, V, loop), _rel(s_losses.cpu().double().numpy(), V[loop + "_losses"]),
         _rel(s_norms.cpu().double().numpy(), V[loop + "_norms"]))
    model, losses, norms, meters = _run_drop_in(M, V, loop, ours)
    assert len(losses) == 12 == meters["steps"]
    d = (PU.max_state_diff(model, V, loop), _rel(losses, V[loop + "_losses"]), _rel(norms, V[loop + "_norms"]))
    print("E2E %s %s: stock torch here vs fixture N = param %.4e loss %.4e norm %.4e | drop-in vs fixture: param %.4e loss %.4e "
          "norm %.4e | drop-in vs stock here: param %.4e" % ((c, loop) + N + d + (_state_diff(model, stock),)))
    assert N[0] <= CHAOS_LIMIT
    for got, n in zip(d, N):
        assert got <= 4 * max(n, SAME_DEVICE_FLOOR)
    # the fused path ran: the meters were kept on the device by the launch pair
    sizes = np.array([len(b3) for b3, _ in PU.batches_of(V, loop)], dtype=np.float64)
    per = np.float32(losses).astype(np.float64).reshape(-1, 4)    # plain, playback, flip, flip + playback per batch
    assert meters["loss"] == pytest.approx(float(np.sum(per[:, 0] * sizes) / np.sum(sizes)), rel=1e-12)
    assert meters["flip_loss"] == meters["loss"] and meters["loss_poses"] == int(sizes.sum())
    # the same call sequence (host numpy batches in the video loop): the same bits
    again, l2, n2, _ = _run_drop_in(M, V, loop, ours, numpy_batches=(loop == "video"))
    assert _state_diff(model, again) == 0 and np.array_equal(losses, l2) and np.array_equal(norms, n2)


def test_three_dimensional_output_under_n_mpjpe_raises(M, G, clips):
    V = CU.loop_view(G, clips, "n", "video")
    model = PU.load_initial(MU.make_model("video"), V, "video").cuda().train()
    run = M.T.StepRunner(model, M.T.posenet_optimizer(model, PU.LR), M.loss.n_mpjpe, torch.device("cuda"))
    assert run.fused == "n_mpjpe"
    b3, b2 = dev(V["v_b3d"][:8]), dev(V["v_b2d"][:8])

    class Flat(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x).view(-1, 16, 3)

    run.step(b2, b3, "loss", 8)                                   # the 4-D form goes through
    assert run.finish(False)["loss_steps"] == 1
    other = Flat(PU.load_initial(MU.make_model("video"), V, "video")).cuda().train()
    flat = M.T.StepRunner(other, M.T.posenet_optimizer(other, PU.LR), M.loss.n_mpjpe, torch.device("cuda"))
    with pytest.raises(ValueError, match="B, F, 16, 3"):
        flat.step(b2, b3.view(-1, 16, 3), "loss", 8)


# ------------------------------------------------------------------------------------------------------------ host reads
def test_fused_epochs_read_the_host_no_more_than_the_mpjpe_epoch(M, G, clips):
    from test_gpu_posetrain import _Count
    V = CU.loop_view(G, clips, "n", "video")
    b3, b2 = dev(V["v_b3d"]), dev(V["v_b2d"])
    reads = {}
    for name, crit in (("mpjpe", M.loss.mpjpe), ("n_mpjpe", M.loss.n_mpjpe), ("wmpjpe", M.loss.JointWeightedMpjpe(CU.LOOP_W16))):
        model = PU.load_initial(MU.make_model("video"), V, "video").cuda()
        opt = M.T.posenet_optimizer(model, 1e-4)
        n = []
        for nb in (3, 30):
            batches = [(b3[(8 * b) % 128:(8 * b) % 128 + 32], b2[(8 * b) % 128:(8 * b) % 128 + 32]) for b in range(nb)]
            loader = PU.loader_of("video", batches)
            M.V.video_mode_train_posenet(model, loader, opt, crit, torch.device("cuda"), PU.loop_args())    # warm-up
            with _Count() as c:
                M.V.video_mode_train_posenet(model, loader, opt, crit, torch.device("cuda"), PU.loop_args())
            assert M.V.video_mode_train_posenet.last_meters["steps"] == 4 * nb
            n.append(c.n)
        reads[name] = n
    print("host reads", reads)
    for name in ("n_mpjpe", "wmpjpe"):
        assert reads[name][0] == reads[name][1] and reads[name][0] <= reads["mpjpe"][0] and reads[name][1] <= reads["mpjpe"][1]


# ----------------------------------------------------------------------------------------------------------------- graph
def _graph_pair(M, name, criterion):
    """(eager run, graph run) of test_gpu_posenet_graph's small model `name`, three epochs each from the same seed"""
    import test_gpu_posenet_graph as TG
    MG = argparse.Namespace(T=M.T, mpjpe=M.loss.mpjpe)
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    from dhaug_amd.models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModelOptimized1f
    MG.Single, MG.Multi = TemporalModelOptimized1f, multiFrame_TemporalModelOptimized1f
    out = []
    for graph in (False, True):
        r = TG.Run(MG, name, "bf16x6", "mse", False)              # (the criterion and the mode are set below, before any step)
        r.criterion, r.graph = criterion, graph
        for _ in range(TG.EPOCHS):
            r.epoch()
        out.append((r, r.state()))
    return out


@pytest.mark.parametrize("c", ["n", "w16"])
def test_graph_run_is_the_launch_by_launch_run(M, c):
    """StepRunner(graph=True) with each new criterion, three epochs: parameters, moments, buffers, per-step losses and norms
    bit-identical to the launch-by-launch loop from the same seed.  The weighted criterion runs on the small `videopose` model of
    tests/test_gpu_posenet_graph.py; n_mpjpe needs a (B, F, 16, 3) output, which that model does not give, and runs on that file's
    small multi-frame model."""
    name = "mulit_farme_videopose" if c == "n" else "videopose"
    crit = M.loss.n_mpjpe if c == "n" else M.loss.JointWeightedMpjpe(CU.LOOP_W16)
    (ea, sa), (gr, sg) = _graph_pair(M, name, crit)
    assert set(sa) == set(sg)
    for k in sorted(sa):
        assert sa[k].dtype == sg[k].dtype and torch.equal(sa[k], sg[k]), k
        assert not sa[k].dtype.is_floating_point or bool(torch.isfinite(sg[k]).all()), k
    assert gr.runners[-1].captures >= 1 and sum(r.replayed_steps for r in gr.runners) > 0
    assert sum(r.replayed_steps for r in ea.runners) == 0 and ea.runners[-1].captures == 0
    for e in range(len(gr.meters)):
        assert gr.meters[e] == ea.meters[e]
    if c == "w16":
        # the captured launch reads the weights in place: a rebuilt criterion (a fresh buffer) is a new key and a new capture
        before = gr.runners[-1].captures
        fresh = M.loss.JointWeightedMpjpe(CU.LOOP_W16)
        gr.criterion = fresh
        run = gr.epoch()
        assert fresh.weights.data_ptr() != crit.weights.data_ptr()
        assert run.eager_steps >= 2 and run.captures == before + 1
        gr.criterion = crit                                       # the old graphs are still there, and are replayed
        again = gr.epoch()
        assert again.eager_steps == 0 and again.replayed_steps == 4 and again.captures == before + 1


def test_graph_refusals_and_3d_n_mpjpe(M):
    import test_gpu_posenet_graph as TG
    from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    MG = argparse.Namespace(Single=TemporalModelOptimized1f)
    model = TG.build(MG, "videopose").cuda().train()
    opt = M.T.posenet_optimizer(model, 1e-3)
    for crit in (M.loss.weighted_mpjpe, M.loss.mpjpe_byjoint, lambda a, b: M.loss.n_mpjpe(a, b)):
        with pytest.raises(ValueError, match="four fused criteria"):
            M.T.StepRunner(model, opt, crit, torch.device("cuda"), graph=True)
    run = M.T.StepRunner(model, opt, M.loss.n_mpjpe, torch.device("cuda"), graph=True)      # accepted ...
    x, t = TG.batches_of("videopose")[0]
    with pytest.raises(ValueError, match="B, F, 16, 3"):                                     # ... and a 3-D output is n_mpjpe's error
        run.step(x, t, "loss", x.shape[0])
    assert not torch.cuda.is_current_stream_capturing()
