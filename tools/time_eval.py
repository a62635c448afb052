"""Device-side posenet evaluation (function_aug/model_pos_eval.evaluate, utils.loss) on an H36M-sized synthetic test set:
531 batches of 1 024 poses (543 744 poses, about S9 + S11 through four cameras), batches already on the device.

  (a) evaluate() per call, host clock (it ends with its one host read): with a two-layer MLP stub posenet on the device, and
      with a null posenet (returns a stored output: the metric part alone); flip + PCK / AUC on and off
  (b) the metric kernel (dhaug_pose_metrics + its reduction) with HIP events: one 1 024-pose batch, and all 543 744 poses in
      one call; bytes read (2 x 192 B per pose) over that time
  (c) --part k: only the kernel launches of (b), for `rocprofv3 --kernel-trace --stats -- python tools/time_eval.py --part k`

    python tools/time_eval.py [--part ab|k] [--reps 5]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import dhaug_amd  # noqa: F401
from dhaug_amd import ops
from dhaug_amd.function_aug import model_pos_eval as ME
from dhaug_amd.utils.loss import AUC_THRESHOLDS
import eval_util as EU

NB, B = 531, 1024
HBM_PEAK = 8.0e12           # MI355X HBM3E, bytes / s


class NullPosenet(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out[:x.shape[0]]


def data():
    g = torch.Generator(device="cuda").manual_seed(0)
    t3 = torch.randn(NB * B, 16, 3, device="cuda", generator=g) * 0.25
    i2 = torch.randn(NB * B, 16, 2, device="cuda", generator=g) * 0.3
    return [(t3[i * B:(i + 1) * B], i2[i * B:(i + 1) * B]) for i in range(NB)], t3


def part_a(batches, reps):
    mlp = EU.StubPosenet(EU.posenet_weights()).cuda()
    null = NullPosenet(torch.randn(B, 48, device="cuda") * 0.25)
    for name, net in (("mlp", mlp), ("null", null)):
        for flip, pck in (("", False), ("_flip", True)):
            ME.evaluate(batches[:4], net, torch.device("cuda"), flipaug=flip, get_pck_auc=pck)
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ME.evaluate(batches, net, torch.device("cuda"), flipaug=flip, get_pck_auc=pck)
                ts.append((time.perf_counter() - t0) * 1e3)
            print("evaluate posenet=%-4s flip=%-5s pck_auc=%d: %.2f ms per call (median of %d; %d batches of %d)"
                  % (name, flip or "-", pck, float(np.median(ts)), reps, NB, B), flush=True)


def kernel_runs(t3, n_small, n_big):
    y = t3 + 0.05
    tot = ops.eval_totals()
    for _ in range(n_small):
        ops.pose_metrics(y[:B], t3[:B], center=True, thresholds=AUC_THRESHOLDS, totals=tot)
    for _ in range(n_big):
        ops.pose_metrics(y, t3, center=True, thresholds=AUC_THRESHOLDS, totals=tot)
    torch.cuda.synchronize()


def part_b(t3, reps):
    y = t3 + 0.05
    tot = ops.eval_totals()
    for P, n in ((B, 200), (NB * B, 20)):
        for _ in range(3):
            ops.pose_metrics(y[:P], t3[:P], center=True, thresholds=AUC_THRESHOLDS, totals=tot)
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                ops.pose_metrics(y[:P], t3[:P], center=True, thresholds=AUC_THRESHOLDS, totals=tot)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / n)
        t = float(np.median(ts))
        nbytes = P * 2 * 192
        print("pose_metrics P=%d: %.1f us per call (events, launches back to back); %.1f MB read, %.2f TB/s = %.1f %% of "
              "HBM peak" % (P, t * 1e3, nbytes / 1e6, nbytes / (t * 1e-3) / 1e12, 100 * nbytes / (t * 1e-3) / HBM_PEAK),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    batches, t3 = data()
    if "a" in a.part:
        part_a(batches, a.reps)
    if "b" in a.part:
        part_b(t3, a.reps)
    if "k" in a.part:
        kernel_runs(t3, 50, 10)
        print("kernel runs done: 50 x P=%d, 10 x P=%d" % (B, NB * B))


if __name__ == "__main__":
    main()
