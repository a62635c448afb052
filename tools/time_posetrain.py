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

  (a) per-batch time (two steps) with HIP events around one epoch of --batches batches: >= 20 warm-up steps, five blocks of
      >= 100 timed steps, median of the blocks
  (b) --part k: one epoch only, no warm-up, for  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_posetrain.py --part k
      --model M --path P --batches N   (launches per step = the difference of two runs with different N over the steps)

    python tools/time_posetrain.py [--part a|k] [--model stub|wide|both] [--path fast|stock|torch|all] [--batches 50]
                                   [--criterion mse|mpjpe]"""
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
from dhaug_amd.utils.loss import mpjpe
import posetrain_util as PU

B = 1024


class WideMLP(nn.Module):
    """Linear(32 -> W, no bias) BN ReLU, `blocks` residual blocks of two (Linear(W -> W, no bias) BN ReLU), Linear(W -> 48)"""

    def __init__(self, width=1024, blocks=4):
        super().__init__()
        layer = lambda i: nn.Sequential(nn.Linear(i, width, bias=False), nn.BatchNorm1d(width), nn.ReLU())
        self.stem = layer(32)
        self.blocks = nn.ModuleList([nn.Sequential(layer(width), layer(width)) for _ in range(blocks)])
        self.head = nn.Linear(width, 48)

    def forward(self, x):
        y = self.stem(x.reshape(x.shape[0], -1))
        for b in self.blocks:
            y = y + b(y)
        return self.head(y).view(-1, 16, 3)


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


def make(model_name, path):
    torch.manual_seed(0)
    model = (PU.StubPosenet() if model_name == "stub" else WideMLP()).cuda()
    opt = T.posenet_optimizer(model, 1e-4) if path == "fast" else torch.optim.Adam(model.parameters(), lr=1e-4)
    return model, opt


def epoch_fn(model_name, path, nb, criterion="mse"):
    g = torch.Generator(device="cuda").manual_seed(1)
    t3 = torch.randn(nb * B, 16, 3, device="cuda", generator=g)
    i2 = torch.randn(nb * B, 16, 2, device="cuda", generator=g) * 0.4
    model, opt = make(model_name, path)
    args, device = PU.loop_args(), torch.device("cuda")
    as_list = [(t3[i * B:(i + 1) * B], i2[i * B:(i + 1) * B], None, None) for i in range(nb)]
    if path == "fast":
        loader, crit = TensorLoader([t3, i2], B), (nn.MSELoss(reduction="mean") if criterion == "mse" else mpjpe)
        return model, lambda: T.train_posenet(model, loader, opt, crit, device, args)
    if path == "stock":
        crit = Wrapped() if criterion == "mse" else torch_mpjpe
        return model, lambda: T.train_posenet(model, as_list, opt, crit, device, args)
    crit = nn.MSELoss(reduction="mean") if criterion == "mse" else torch_mpjpe
    pairs = [(a, b) for a, b, _, _ in as_list]
    return model, lambda: PU.stock_loop(model, "single", pairs, opt, crit, use_flip=True)


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
    ap.add_argument("--criterion", choices=("mse", "mpjpe"), default="mse")
    a = ap.parse_args()
    models = ["stub", "wide"] if a.model == "both" else [a.model]
    paths = ["fast", "stock", "torch"] if a.path == "all" else [a.path]
    T.summary_line = lambda *x, **k: None                        # one line per epoch would drown the report
    if a.part == "a":
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
