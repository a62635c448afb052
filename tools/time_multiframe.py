"""The video mode's posenet with the package's own classes (models_Fk_GAN/mulit_farme_videopose.py), C = 1 024, dropout 0.25.

Training: one optimizer step through function_aug.model_pos_train.StepRunner (forward, MSE, backward, clip, Adam with PosenetAdam)
on B = 512 clips of one receptive field, architectures '3,3' (9 frames) and '3,3,3' (27 frames).  Variants:
  bf16, bf16x6    multiFrame_TemporalModelOptimized1f in that precision;
  stock           the same network from stock nn.Conv1d / nn.BatchNorm1d modules in fp32 (tests/multiframe_util.StockMultiFrame): what a
                  user of the video mode runs without this package's classes;
  bf16-permute,   our class with the tap kernels (dhaug_conv_taps_pack_bf16, dhaug_conv_taps_permute_f32) replaced by torch's
  bf16x6-permute  permute().contiguous() in front of the existing cast / transpose kernels and on the weight gradient.  Built here, by
                  swapping the two ops wrappers while the variant runs; the library has no such switch.
Evaluation: multiFrame_TemporalModel on one sequence of 2 000 frames (gradients off) against the stock dilated module.

All variants of a workload run in ONE process, warmed up, then alternating: --rounds rounds (at least five), each variant --steps steps
per round between HIP events; the median of a variant's rounds is reported.

--graph: the training side alone, variants "<precision>", "<precision>+graph" (StepRunner(graph=True): the step replayed as a hipGraph)
and the stock module.

    python tools/time_multiframe.py [--steps 20] [--rounds 5] [--arch 3,3 --arch 3,3,3] [--graph]"""
import argparse
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn as nn

import dhaug_amd  # noqa: F401
from dhaug_amd import ops
from dhaug_amd.function_aug import model_pos_train as T
from dhaug_amd.models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModel, multiFrame_TemporalModelOptimized1f
import multiframe_util as MU

B, C, EVAL_FRAMES = 512, 1024, 2000
TRAIN_VARIANTS = ("bf16", "bf16x6", "stock", "bf16-permute", "bf16x6-permute")
EVAL_VARIANTS = ("bf16", "bf16x6", "stock")
GRAPH_VARIANTS = ("bf16", "bf16+graph", "bf16x6", "bf16x6+graph", "stock")


@contextlib.contextmanager
def torch_permute():
    """the two tap kernels replaced by torch permutes (each a read and a write of the whole weight) in front of the existing kernels"""
    pack, permute = ops.conv_taps_pack_bf16, ops.conv_taps_permute_f32

    def pack_torch(W, want_nn=True, nt=None, nn=None):
        W2d = W.permute(0, 2, 1).contiguous().view(W.shape[0], -1)
        return ops.cast_pad_bf16(W2d, W2d.shape[1]), (ops.cast_transpose_bf16(W2d) if want_nn else None)

    def permute_torch(src, N, Cin, k, to_taps, out=None, accumulate=False):
        assert out is None and not accumulate
        if to_taps:
            return src.view(N, Cin, k).permute(0, 2, 1).contiguous().view(N, k * Cin)
        return src.view(N, k, Cin).permute(0, 2, 1).contiguous()

    ops.conv_taps_pack_bf16, ops.conv_taps_permute_f32 = pack_torch, permute_torch
    try:
        yield
    finally:
        ops.conv_taps_pack_bf16, ops.conv_taps_permute_f32 = pack, permute


def train_fn(variant, arch, steps):
    g = torch.Generator(device="cuda").manual_seed(1)
    rf = MU.receptive_field(arch)
    x = torch.randn(B, rf, 16, 2, device="cuda", generator=g) * 0.4
    t = torch.randn(B, 1, 16, 3, device="cuda", generator=g) * 0.3
    torch.manual_seed(0)
    variant, _, graph = variant.partition("+")
    if variant == "stock":
        model = MU.StockMultiFrame(C, arch, True, dropout=0.25).cuda()
    else:
        model = multiFrame_TemporalModelOptimized1f(16, 2, 16, filter_widths=list(arch), dropout=0.25, channels=C).cuda()
        model.precision = variant.split("-")[0]
    model.train()
    runner = T.StepRunner(model, T.posenet_optimizer(model, 1e-4), nn.MSELoss(reduction="mean"), torch.device("cuda"),
                          graph=bool(graph))
    ctx = torch_permute if variant.endswith("-permute") else contextlib.nullcontext

    def run():
        with ctx():
            for _ in range(steps):
                runner.step(x, t, None, B)
    return run


def eval_fn(variant, arch, steps):
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(1, EVAL_FRAMES, 16, 2, device="cuda", generator=g) * 0.4
    torch.manual_seed(0)
    if variant == "stock":
        model = MU.StockMultiFrame(C, arch, False).cuda()
    else:
        model = multiFrame_TemporalModel(16, 2, 16, filter_widths=list(arch), channels=C).cuda()
        model.precision = variant
    model.eval()

    def run():
        with torch.no_grad():
            for _ in range(steps):
                model(x)
    return run


def measure(title, variants, make, arch, steps, rounds):
    runs = {v: make(v, arch, steps) for v in variants}
    for run in runs.values():
        run()                                                     # warm-up: `steps` steps each
    ts = {v: [] for v in variants}
    for _ in range(rounds):
        for v, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ts[v].append(e0.elapsed_time(e1) / steps)
    for v in variants:
        print("%s arch=%s %-15s: %.3f ms (median of %d alternating rounds of %d; rounds %s)"
              % (title, ",".join(str(w) for w in arch), v, float(np.median(ts[v])), rounds, steps, " ".join("%.3f" % t for t in ts[v])),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arch", action="append")
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5 (the median of fewer blocks is not reported)")
    for arch in (a.arch or ["3,3", "3,3,3"]):
        arch = tuple(int(w) for w in arch.split(","))
        measure("train step B=%d" % B, GRAPH_VARIANTS if a.graph else TRAIN_VARIANTS, train_fn, arch, a.steps, a.rounds)
        if a.graph:
            continue
        measure("eval %d frames" % EVAL_FRAMES, EVAL_VARIANTS, eval_fn, arch, a.steps, a.rounds)


if __name__ == "__main__":
    main()
