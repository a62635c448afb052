"""The MLP posenet (models_baseline.mlp.LinearModel) at B = 1 024, C = 1 024, stages 2 and 4, dropout 0.25, against its stock
restatement (tests/linear_model_util.StockMLP: nn.Linear / nn.BatchNorm1d / nn.Dropout under the same names, fp32).

  training    one StepRunner step (forward, dhaug_pose_mse, backward, clip + Adam) with PosenetAdam in 'bf16', 'bf16x3' and 'bf16x6';
              the comparison is the stock container under the same StepRunner with torch.optim.Adam (clip_grad_norm_ + step)
  evaluation  the evaluation forward (gradients off, folded operands cached) in the three precisions against the stock module's

All variants of a side run in ONE process, warmed up, then alternating: five rounds of 50 calls per variant between HIP events; the
median of a variant's five rounds is reported.  Reported, not gated.

--graph: the training side alone, with a third line per precision: "<precision>+graph" = StepRunner(graph=True), the step replayed as a
hipGraph, beside the launch-by-launch step and the stock module.

    python tools/time_linear_model.py [--calls 50] [--graph]"""
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
from dhaug_amd.models_baseline.mlp import LinearModel, init_weights
import linear_model_util as LU

B, C, DROPOUT = 1024, 1024, 0.25
VARIANTS = ("stock", "bf16", "bf16x3", "bf16x6")
GRAPH_VARIANTS = ("stock",) + tuple(v + s for v in VARIANTS[1:] for s in ("", "+graph"))


def build(variant, stages):
    torch.manual_seed(0)
    if variant == "stock":
        return LU.StockMLP(C, stages, DROPOUT).apply(init_weights).cuda()
    model = LinearModel(32, 45, linear_size=C, num_stage=stages, p_dropout=DROPOUT).apply(init_weights).cuda()
    model.precision = variant
    return model


def train_fn(variant, stages, x, t):
    variant, _, graph = variant.partition("+")
    model = build(variant, stages).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4) if variant == "stock" else T.posenet_optimizer(model, 1e-4)
    run = T.StepRunner(model, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"), graph=bool(graph))

    return lambda: run.step(x, t, "loss", B)


def eval_fn(variant, stages, x, t):
    model = build(variant, stages).eval()

    def forward():
        with torch.no_grad():
            model(x)
    return forward


def measure(fns, calls):
    for f in fns.values():
        for _ in range(10):
            f()
    ts = {v: [] for v in fns}
    for _ in range(5):
        for v, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            e1.synchronize()
            ts[v].append(e0.elapsed_time(e1) / calls * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 16, 2, device="cuda", generator=g) * 0.4
    t = torch.randn(B, 16, 3, device="cuda", generator=g) * 0.3
    t[:, 0] = 0
    for stages in (2, 4):
        for side, make in (("training step", train_fn), ("evaluation forward", eval_fn))[:1 if a.graph else 2]:
            variants = GRAPH_VARIANTS if a.graph else VARIANTS
            ts = measure({v: make(v, stages, x, t) for v in variants}, a.calls)
            stock = float(np.median(ts["stock"]))
            for v in variants:
                med = float(np.median(ts[v]))
                print("mlp stages=%d %-18s %-12s: %8.1f us (%.2f x stock; median of 5 alternating rounds of %d; rounds %s)"
                      % (stages, side, v, med, med / stock, a.calls, " ".join("%.1f" % r for r in ts[v])), flush=True)


if __name__ == "__main__":
    main()
