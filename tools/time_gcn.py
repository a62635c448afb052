"""The SemGCN posenet's training step and evaluation forward at batch 1 024, hid 128, 4 blocks, dropout 0.25.

Variants: "stock" = the plain-torch restatement of tests/gcn_util.py (StockGCN, fp32), and models_baseline.gcn.SemGCN in each
precision ("bf16", "bf16x3", "bf16x6").  Every variant takes its steps through function_aug.model_pos_train.StepRunner with the fused
loss and PosenetAdam, so the difference between two lines is the network's forward and backward alone.

All variants in ONE process, warmed up, then alternating: five rounds, every variant --steps training steps (and --steps evaluation
forwards under no_grad) per round between HIP events on the stream; the median of a variant's five rounds is reported, with the
rounds behind it.  No speed is promised: the network has 0.27 M parameters and its step is a chain of small launches.

--graph: the training step alone, with a third line per precision: "<precision>+graph" = StepRunner(graph=True), the step replayed as a
hipGraph, beside the launch-by-launch step and the stock module.

    python tools/time_gcn.py [--steps 50] [--graph]"""
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
from dhaug_amd.models_baseline.gcn import H36M_PARENTS, SemGCN, adj_mx_from_parents
import gcn_util as CU

B, HID, BLOCKS, DROPOUT = 1024, 128, 4, 0.25
VARIANTS = ("stock", "bf16", "bf16x3", "bf16x6")
GRAPH_VARIANTS = ("stock",) + tuple(v + s for v in VARIANTS[1:] for s in ("", "+graph"))


def build(variant):
    torch.manual_seed(0)
    if variant == "stock":
        return CU.StockGCN(HID, BLOCKS, DROPOUT).cuda()
    model = SemGCN(adj_mx_from_parents(H36M_PARENTS), HID, num_layers=BLOCKS, p_dropout=DROPOUT).cuda()
    model.precision = variant
    return model


def runners(variant, steps):
    """(train, evaluate): `steps` optimizer steps / `steps` evaluation forwards on fixed device batches"""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 16, 2, device="cuda", generator=g) * 0.4
    t = torch.randn(B, 16, 3, device="cuda", generator=g) * 0.3
    variant, _, graph = variant.partition("+")
    model = build(variant)
    if graph:
        model.train()
    run = T.StepRunner(model, T.posenet_optimizer(model, 1e-4), nn.MSELoss(reduction="mean"), torch.device("cuda"), graph=bool(graph))

    def train():
        model.train()
        with torch.enable_grad():
            for _ in range(steps):
                run.step(x, t, "loss", B)

    def evaluate():
        model.eval()
        with torch.no_grad():
            for _ in range(steps):
                model(x)

    return train, evaluate


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_gcn.py needs a GPU: a time taken anywhere else says nothing")
    variants = GRAPH_VARIANTS if a.graph else VARIANTS
    runs = {v: runners(v, a.steps) for v in variants}
    for train, evaluate in runs.values():                           # warm-up: every shape the timed windows use
        train(), evaluate()
    ts = {(v, k): [] for v in variants for k in ("train", "eval")}
    for _ in range(5):
        for v, (train, evaluate) in runs.items():
            ts[(v, "train")].append(timed(train) / a.steps)
            if not a.graph:
                ts[(v, "eval")].append(timed(evaluate) / a.steps)
    sides = (("train", "training step (forward, loss, backward, clip + Adam)"), ("eval", "evaluation forward"))
    for k, what in sides[:1 if a.graph else 2]:
        for v in variants:
            r = ts[(v, k)]
            print("gcn=%-12s: %.3f ms per %s at B = %d (median of 5 alternating rounds of %d; rounds %s)"
                  % (v, float(np.median(r)), what, B, a.steps, " ".join("%.3f" % q for q in r)), flush=True)


if __name__ == "__main__":
    main()
