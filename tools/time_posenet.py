"""The posenet's training step with the package's own model: train_posenet + PosenetAdam at batch 1 024, flip on (one plain + one
flipped optimizer step per batch), pairs on the device, C = 1 024, stages 4, dropout 0.25.

Variants: "stock" = the plain-torch wide BatchNorm MLP of tools/time_posetrain.py (what DESIGN.md section 4.5 measured), and
models_baseline.videopose.TemporalModelOptimized1f in each precision ("bf16", "bf16x3", "bf16x6").

  (a) per-batch time: all variants in ONE process, warmed up, then alternating -- five rounds, every variant one epoch of
      --batches batches (100 steps) per round between HIP events; the median of a variant's five epochs is reported
  (b) launches per optimizer step: a rocprofv3 --kernel-trace --stats run of this file (--part k) per variant at two epoch lengths
      in child processes; (calls(N2) - calls(N1)) / (2 (N2 - N1)) leaves the start-up launches out

  --graph: part (a) alone, with a third line per precision: "<precision>+graph" = the same loop with args.posenet_graph (the step
      replayed as a hipGraph, function_aug.model_pos_train.StepRunner(graph=True)) beside the launch-by-launch loop and the stock module

    python tools/time_posenet.py [--batches 50] [--no-launches] [--graph]"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import torch.nn as nn

import dhaug_amd  # noqa: F401
from dhaug_amd.function_aug import model_pos_train as T
from dhaug_amd.function_aug.dataloader_update import TensorLoader
from dhaug_amd.models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
import posetrain_util as PU
from time_posetrain import WideMLP

B = 1024
VARIANTS = ("stock", "bf16", "bf16x3", "bf16x6")
GRAPH_VARIANTS = ("stock",) + tuple(v + s for v in VARIANTS[1:] for s in ("", "+graph"))


def epoch_fn(variant, nb):
    g = torch.Generator(device="cuda").manual_seed(1)
    t3 = torch.randn(nb * B, 16, 3, device="cuda", generator=g)
    i2 = torch.randn(nb * B, 16, 2, device="cuda", generator=g) * 0.4
    torch.manual_seed(0)
    variant, _, graph = variant.partition("+")
    if variant == "stock":
        model = WideMLP().cuda()
    else:
        model = TemporalModelOptimized1f(16, 2, 15, filter_widths=[1] * 5, dropout=0.25, channels=1024).cuda()
        model.precision = variant
    opt = T.posenet_optimizer(model, 1e-4)
    loader, crit, args, device = TensorLoader([t3, i2], B), nn.MSELoss(reduction="mean"), PU.loop_args(), torch.device("cuda")
    args.posenet_graph = bool(graph)
    return lambda: T.train_posenet(model, loader, opt, crit, device, args)


def part_a(nb, variants=VARIANTS):
    runs = {v: epoch_fn(v, nb) for v in variants}
    for run in runs.values():
        run()                                                     # warm-up: 2 nb steps each (a graph variant captures its two steps here)
    ts = {v: [] for v in variants}
    for _ in range(5):
        for v, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ts[v].append(e0.elapsed_time(e1) / nb)
    for v in variants:
        print("posenet=%-12s: %.3f ms per batch of %d = plain + flipped step (median of 5 alternating epochs of %d steps; epochs %s)"
              % (v, float(np.median(ts[v])), B, 2 * nb, " ".join("%.3f" % t for t in ts[v])), flush=True)


def kernel_calls(variant, nb):
    """kernel launches of one child run under rocprofv3 (--part k: one epoch, no warm-up)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--part", "k", "--variant", variant, "--batches", str(nb)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stdout[-2000:])
        total = 0
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(f) as fh:
                total += sum(int(row["Calls"]) for row in csv.DictReader(fh))
        return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="a")
    ap.add_argument("--variant", default="stock")
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    T.summary_line = lambda *x, **k: None                        # one line per epoch would drown the report
    if a.part == "k":
        epoch_fn(a.variant, a.batches)()
        torch.cuda.synchronize()
        return
    part_a(a.batches, GRAPH_VARIANTS if a.graph else VARIANTS)
    if not a.no_launches and not a.graph:
        n1, n2 = 4, 12
        for v in VARIANTS:
            c1, c2 = kernel_calls(v, n1), kernel_calls(v, n2)
            print("posenet=%-6s: %.1f launches per optimizer step (%d and %d kernel calls at %d and %d steps)"
                  % (v, (c2 - c1) / (2.0 * (n2 - n1)), c1, c2, 2 * n1, 2 * n2), flush=True)


if __name__ == "__main__":
    main()
