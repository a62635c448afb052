"""The PoseFormer posenet (models_baseline.poseformer.PoseTransformer) at the reference's configuration (16 joints, ratio 32, depth 4,
8 heads), B = 512 clips of 9 and of 27 frames, against its stock restatement (tests/poseformer_util.StockPoseFormer: nn.Linear /
nn.LayerNorm under the same names, F.gelu, softmax attention written out, fp32).  Drop path 0 on both sides.

  training    one StepRunner step (forward, dhaug_pose_mse, backward, clip + Adam) with PosenetAdam in 'bf16', 'bf16x3' and 'bf16x6';
              the comparison is the stock container under the same StepRunner with torch.optim.Adam (clip_grad_norm_ + step)
  evaluation  the evaluation forward (gradients off) in the three precisions against the stock module's
  attention   dhaug_attn_forward and dhaug_attn_forward + dhaug_attn_backward alone, fp32 and bf16, against the torch expression they
              replace (reshape, permute, two batched matmuls, scale, softmax; autograd for the backward) at the two spatial shapes

All variants of a side run in ONE process, warmed up, then alternating: five rounds of 50 calls per variant between HIP events; the
median of a variant's five rounds is reported.  Reported, not gated.

    python tools/time_poseformer.py [--calls 50] [--clips 512]"""
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
from dhaug_amd import ops
from dhaug_amd.function_aug import model_pos_train as T
from dhaug_amd.models_baseline.mlp import init_weights
from dhaug_amd.models_baseline.poseformer import PoseTransformer
import poseformer_util as FU

VARIANTS = ("stock", "bf16", "bf16x3", "bf16x6")


def build(variant, frames):
    torch.manual_seed(0)
    cfg = FU.reference_cfg(frames)
    if variant == "stock":
        return FU.StockPoseFormer(**{k: v for k, v in cfg.items() if k != "seed"}).apply(init_weights).cuda()
    model = PoseTransformer(**FU.kwargs(cfg)).apply(init_weights).cuda()
    model.precision = variant
    return model


def train_fn(variant, frames, x, t):
    model = build(variant, frames).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4) if variant == "stock" else T.posenet_optimizer(model, 1e-4)
    run = T.StepRunner(model, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"))
    return lambda: run.step(x, t, "loss", x.shape[0])


def eval_fn(variant, frames, x, t):
    model = build(variant, frames).eval()

    def forward():
        with torch.no_grad():
            model(x)
    return forward


def attention_fns(S, N, H, hd, backward):
    C, scale = H * hd, hd ** -0.5
    g = torch.Generator(device="cuda").manual_seed(2)
    qkv = torch.randn(S * N, 3 * C, device="cuda", generator=g)
    gout = torch.randn(S * N, C, device="cuda", generator=g)
    fns = {}

    def stock():
        leaf = qkv.detach().requires_grad_(backward)
        q, k, v = leaf.view(S, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        out = (((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1) @ v).transpose(1, 2).reshape(S * N, C)
        if backward:
            out.backward(gout)
    fns["stock"] = stock
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        a, b = qkv.to(dtype), gout.to(dtype)

        def ours(a=a, b=b):
            out, lse = ops.attn_forward(a, S, N, H, hd, scale)
            if backward:
                ops.attn_backward(a, out, lse, b, S, N, H, hd, scale)
        fns[name] = ours
    return fns


def measure(fns, calls):
    for f in fns.values():
        for _ in range(5):
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


def report(what, ts, calls):
    stock = float(np.median(ts["stock"]))
    for v in ts:
        med = float(np.median(ts[v]))
        print("poseformer %-34s %-6s: %9.1f us (%.2f x stock; median of 5 alternating rounds of %d; rounds %s)"
              % (what, v, med, med / stock, calls, " ".join("%.1f" % r for r in ts[v])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--clips", type=int, default=512)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    B = a.clips
    for frames in (9, 27):
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, frames, 16, 2, device="cuda", generator=g) * 0.4
        t = torch.randn(B, 1, 16, 3, device="cuda", generator=g) * 0.3
        for side, make in (("training step", train_fn), ("evaluation forward", eval_fn)):
            report("B=%d frames=%d %s" % (B, frames, side), measure({v: make(v, frames, x, t) for v in VARIANTS}, a.calls), a.calls)
        for backward in (False, True):
            what = "attention %s S=%d N=16 H=8 hd=4" % ("fwd+bwd" if backward else "forward", B * frames)
            report(what, measure(attention_fns(B * frames, 16, 8, 4, backward), a.calls), a.calls)


if __name__ == "__main__":
    main()
