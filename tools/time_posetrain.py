"""Posenet training steps (function_aug/model_pos_train.train_posenet) at batch 1 024, flip on: one plain + one flipped
optimizer step per batch, pairs already on the device.

Posenets: "stub" (tests/posetrain_util.StubPosenet, 9.3 k parameters: the step is launch-bound) and "wide", a plain-torch
1 024-wide, 4-block BatchNorm MLP of the reference VideoPose network's shape (about 8.4 M parameters).
Paths:
  fast    the drop-in with nn.MSELoss + PosenetAdam over a TensorLoader: dhaug_pair_batch from index slices, dhaug_pose_mse,
          dhaug_grad_sumsq + dhaug_adam_clip_step
  stock   the same drop-in falling back piece by piece: a criterion it does not recognise (MSELoss behind a wrapper), stock
          torch.optim.Adam and nn.utils.clip_grad_norm_, batches from a plain list
  torch   the reference's sequence of calls in plain torch (tests/posetrain_util.stock_loop), batches from a plain list,
          without the reference's per-step .item() -- what a user runs today, minus its host reads
--criterion mpjpe: the criterion of the reference's video command instead of nn.MSELoss.  fast = this package's utils.loss.mpjpe
(dhaug_pose_mpjpe: loss, gradient and meter in one launch pair); stock and torch = the generic path, with the reference's torch
expression mean(norm(predicted - target, dim=-1)) as the criterion (forward + autograd backward).  The paths alternate in one
process, as for MSE.
--criterion wmpjpe: fast = utils.loss.JointWeightedMpjpe (dhaug_pose_wmpjpe, sixteen shared weights); stock and torch = the torch
expression mean(w * norm(predicted - target, dim=-1)) with the weights expanded, on the generic path.
--criterion n_mpjpe: fast = utils.loss.n_mpjpe (dhaug_pose_nmpjpe); stock and torch = the reference's torch expression.  n_mpjpe
takes (B, F, 16, 3), so this criterion runs GAN_dataSet_video_mode_train_posenet on clips of ONE frame (batch 1 024 x 1 frame,
flip on, playback off: the same two steps per batch) with the posenet's output viewed as (B, 1, 16, 3).

  (e) --part e: the three criteria entries alone (ops.pose_nmpjpe, ops.pose_wmpjpe with shared weights: loss + gradient;
      mpjpe_byjoint: dhaug_pose_column_errors forward + ops.pose_byjoint_backward) against torch's forward + autograd backward of
      the expressions they replace, at (1 024, 1, 16, 3) and, for the per-joint table, (512, 243, 16, 3).  The two variants
      alternate call by call in one process; HIP events around each call; per variant the median of five rounds' means.
  (a) per-batch time (two steps) with HIP events around one epoch of --batches batches: >= 20 warm-up steps, five blocks of
      >= 100 timed steps, median of the blocks
  (b) --part k: one epoch only, no warm-up, for  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_posetrain.py --part k
      --model M --path P --batches N   (launches per step = the difference of two runs with different N over the steps)

    python tools/time_posetrain.py [--part a|k|e] [--model stub|wide|both] [--path fast|stock|torch|all] [--batches 50]
                                   [--criterion mse|mpjpe|n_mpjpe|wmpjpe]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn as nn

import dhaug_amd  # noqa: F401
from dhaug_amd.function_aug import model_pos_train as T
from dhaug_amd.function_aug.dataloader_update import TensorLoader
from dhaug_amd import ops
from dhaug_amd.models_Fk_GAN import video_mode_operate as V
from dhaug_amd.utils import loss as LS
from dhaug_amd.utils.loss import mpjpe
import pose_criteria_util as CU
import posetrain_util as PU

B = 1024
CRITERIA = ("mse", "mpjpe", "n_mpjpe", "wmpjpe")


class WideMLP(nn.Module):
    """Linear(32 -> W, no bias) BN ReLU, `blocks` residual blocks of two (Linear(W -> W, no bias) BN ReLU), Linear(W -> 48)"""

    def __init__(self, width=1024, blocks=4):
        super().__init__()
        layer = lambda i: nn.Sequential(nn.Linear(i, width, bias=False), nn.BatchNorm1d(width), nn.ReLU())
        self.stem = layer(32)
        self.blocks = nn.ModuleList([nn.Sequential(layer(width), layer(width)) for _ in range(blocks)])
        self.head = nn.Linear(width, 48)
        self.clips = False                                        # True: the output as (B, 1, 16, 3), what n_mpjpe takes

    def forward(self, x):
        y = self.stem(x.reshape(x.shape[0], -1))
        for b in self.blocks:
            y = y + b(y)
        return self.head(y).view(-1, 1, 16, 3) if self.clips else self.head(y).view(-1, 16, 3)


class Wrapped(nn.Module):
    """nn.MSELoss the drop-in does not recognise"""

    def __init__(self):
        super().__init__()
        self.inner = nn.MSELoss(reduction="mean")

    def forward(self, a, b):
        return self.inner(a, b)


def torch_mpjpe(predicted, target):
    """the reference's mpjpe (R/utils/loss.py:8-14) in stock torch: not the package's function, so the generic path"""
    return torch.mean(torch.norm(predicted - target, dim=len(target.shape) - 1))


def make(model_name, path, clips=False):
    torch.manual_seed(0)
    model = (PU.StubPosenet(1 if clips else 0) if model_name == "stub" else WideMLP()).cuda()
    model.clips = clips
    opt = T.posenet_optimizer(model, 1e-4) if path == "fast" else torch.optim.Adam(model.parameters(), lr=1e-4)
    return model, opt


def criteria_of(criterion):
    """(what the drop-in fuses, a criterion it does not recognise, the plain-torch criterion)"""
    if criterion == "mse":
        return nn.MSELoss(reduction="mean"), Wrapped(), nn.MSELoss(reduction="mean")
    if criterion == "mpjpe":
        return mpjpe, torch_mpjpe, torch_mpjpe
    if criterion == "n_mpjpe":
        return LS.n_mpjpe, CU.torch_n_mpjpe, CU.torch_n_mpjpe
    w16 = torch.from_numpy(CU.LOOP_W16).cuda()
    expanded = lambda p, t: CU.torch_weighted_mpjpe(p, t, w16.expand(p.shape[:-1]))
    return LS.JointWeightedMpjpe(CU.LOOP_W16), expanded, expanded


def epoch_fn(model_name, path, nb, criterion="mse"):
    g = torch.Generator(device="cuda").manual_seed(1)
    t3 = torch.randn(nb * B, 16, 3, device="cuda", generator=g)
    i2 = torch.randn(nb * B, 16, 2, device="cuda", generator=g) * 0.4
    clips = criterion == "n_mpjpe"
    model, opt = make(model_name, path, clips)
    args, device = PU.loop_args(), torch.device("cuda")
    fused, unknown, plain = criteria_of(criterion)
    if clips:                                                     # clips of one frame through the GAN-clips loop, playback off
        t3, i2 = t3.view(-1, 1, 16, 3), i2.view(-1, 1, 16, 2)
        args.GAN_video_playback_input = False
        pairs = [(t3[i * B:(i + 1) * B], i2[i * B:(i + 1) * B]) for i in range(nb)]
        as_list = [(None, a, b) for a, b in pairs]
        if path == "fast":
            loader = TensorLoader([t3, i2], B)
            return model, lambda: V.GAN_dataSet_video_mode_train_posenet(model, loader, opt, fused, device, args)
        if path == "stock":
            return model, lambda: V.GAN_dataSet_video_mode_train_posenet(model, as_list, opt, unknown, device, args)
        return model, lambda: PU.stock_loop(model, "gan", pairs, opt, plain, use_flip=True, playback=False)
    as_list = [(t3[i * B:(i + 1) * B], i2[i * B:(i + 1) * B], None, None) for i in range(nb)]
    if path == "fast":
        loader = TensorLoader([t3, i2], B)
        return model, lambda: T.train_posenet(model, loader, opt, fused, device, args)
    if path == "stock":
        return model, lambda: T.train_posenet(model, as_list, opt, unknown, device, args)
    pairs = [(a, b) for a, b, _, _ in as_list]
    return model, lambda: PU.stock_loop(model, "single", pairs, opt, plain, use_flip=True)


def part_e(rounds=5, reps=50):
    """the three entries alone against torch's forward + backward of the expressions they replace"""
    g = torch.Generator(device="cuda").manual_seed(2)
    w16 = torch.from_numpy(CU.LOOP_W16).cuda()

    def pair(shape):
        t = torch.randn(shape, device="cuda", generator=g)
        return (t * 1.1 + 0.3 * torch.randn(shape, device="cuda", generator=g)), t

    def torch_fb(expr, p, t):
        def run():
            q = p.detach().requires_grad_(True)
            v = expr(q, t)
            (v.sum() if v.dim() else v).backward()
        return run

    def byjoint_kernels(p, t):
        cols = torch.zeros(p[0].numel() // 3, dtype=torch.float64, device="cuda")
        cot = torch.ones(p[0].numel() // 3, device="cuda")

        def run():
            cols.zero_()
            ops.pose_column_errors(p, t, col_sums=cols)
            ops.pose_byjoint_backward(p, t, cot)
        return run

    small, table = pair((B, 1, 16, 3)), pair((512, 243, 16, 3))
    ws = ops.posetrain_workspace()
    cases = [("n_mpjpe (1024, 1, 16, 3)", lambda: ops.pose_nmpjpe(small[0], small[1], B, workspace=ws),
              torch_fb(CU.torch_n_mpjpe, *small)),
             ("weighted_mpjpe, 16 shared weights (1024, 1, 16, 3)", lambda: ops.pose_wmpjpe(small[0], small[1], w16, B, workspace=ws),
              torch_fb(lambda p, t: CU.torch_weighted_mpjpe(p, t, w16.expand(p.shape[:-1])), *small)),
             ("mpjpe_byjoint (1024, 1, 16, 3)", byjoint_kernels(*small), torch_fb(CU.torch_mpjpe_byjoint, *small)),
             ("mpjpe_byjoint (512, 243, 16, 3)", byjoint_kernels(*table), torch_fb(CU.torch_mpjpe_byjoint, *table))]
    for name, ours, theirs in cases:
        for f in (ours, theirs):                                  # warm-up
            for _ in range(5):
                f()
        means = ([], [])
        for _ in range(rounds):
            tot = [0.0, 0.0]
            for _ in range(reps):
                for k, f in enumerate((ours, theirs)):            # the variants alternate call by call
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    tot[k] += e0.elapsed_time(e1)
            for k in (0, 1):
                means[k].append(1e3 * tot[k] / reps)
        print("entry %-52s kernels %8.1f us  torch forward + backward %8.1f us  (median of %d rounds of %d calls; rounds: %s | %s)"
              % (name, float(np.median(means[0])), float(np.median(means[1])), rounds, reps,
                 " ".join("%.1f" % v for v in means[0]), " ".join("%.1f" % v for v in means[1])), flush=True)


def part_a(models, paths, nb, criterion):
    for m in models:
        for p in paths:
            model, run = epoch_fn(m, p, nb, criterion)
            run()                                                 # warm-up: 2 nb steps
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) / nb)
            print("criterion=%-5s posenet=%-4s (%d parameters) path=%-5s: %.3f ms per batch of %d = plain + flipped step (median of 5 epochs of %d "
                  "steps; blocks %s)" % (criterion, m, sum(q.numel() for q in model.parameters()), p, float(np.median(ts)), B, 2 * nb,
                                         " ".join("%.3f" % t for t in ts)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="a")
    ap.add_argument("--model", default="both")
    ap.add_argument("--path", default="all")
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--criterion", choices=CRITERIA, default="mse")
    a = ap.parse_args()
    models = ["stub", "wide"] if a.model == "both" else [a.model]
    paths = ["fast", "stock", "torch"] if a.path == "all" else [a.path]
    T.summary_line = lambda *x, **k: None                        # one line per epoch would drown the report
    if a.part == "e":
        part_e()
    elif a.part == "a":
        part_a(models, paths, a.batches, a.criterion)
    else:
        for m in models:
            for p in paths:
                _, run = epoch_fn(m, p, a.batches, a.criterion)
                run()
                torch.cuda.synchronize()
                print("kernel run done: criterion=%s posenet=%s path=%s, %d steps" % (a.criterion, m, p, 2 * a.batches))


if __name__ == "__main__":
    main()
