"""The detailed pose errors (dhaug_pose_column_errors, dhaug_pose_scaled_errors) against the reference's torch expressions on
the same GPU, at the H36M evaluation-set size of tests/test_gpu_eval.py::test_coverage_at_h36m_scale: 543 744 poses, already on
the device, as (P, 16, 3) and as (P / 243, 243, 16, 3) clips.

Each pair (kernel path, torch expression) alternates in one process; a round is `--calls` back-to-back calls between two HIP
events, the figure the median of `--rounds` rounds after a warm-up of both.  Bytes are what the algorithm reads (2 x 192 B per
pose, plus the weights); the torch expressions read and write several times that in temporaries.  The calls of a round repeat on
the same 209 MB, which fit the 256 MiB Infinity Cache: the TB/s printed is a rate of algorithmic bytes, not an HBM rate.  The
kernel path includes the wrapper's zeroing of its sums and its workspace allocation.  Not a gate: it prints.

    python tools/time_eval_detail.py [--rounds 5] [--calls 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import dhaug_amd  # noqa: F401
from dhaug_amd import ops

P = 531 * 1024
FRAMES = 243


def torch_byjoint(y, x):
    return torch.mean(torch.norm(y - x, dim=-1), dim=0)


def torch_velocity(y, x):
    return torch.mean(torch.norm((y[1:] - y[:-1]) - (x[1:] - x[:-1]), dim=-1))


def torch_weighted(y, x, w):
    return torch.mean(w * torch.norm(y - x, dim=-1))


def torch_n_mpjpe(y, x):
    norm_predicted = torch.mean(torch.sum(y ** 2, dim=3, keepdim=True), dim=2, keepdim=True)
    norm_target = torch.mean(torch.sum(x * y, dim=3, keepdim=True), dim=2, keepdim=True)
    return torch.mean(torch.norm(norm_target / norm_predicted * y - x, dim=-1))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def compare(name, kernel, expr, nbytes, rounds, calls):
    for _ in range(3):
        kernel(), expr()
    tk, te = [], []
    for _ in range(rounds):
        tk.append(timed(kernel, calls))
        te.append(timed(expr, calls))
    k, e = float(np.median(tk)), float(np.median(te))
    print("%-34s kernel %8.1f us [%.1f-%.1f]  torch %8.1f us [%.1f-%.1f]  x%.1f;  %.0f MB read, %.2f TB/s"
          % (name, k * 1e3, min(tk) * 1e3, max(tk) * 1e3, e * 1e3, min(te) * 1e3, max(te) * 1e3, e / k, nbytes / 1e6,
             nbytes / (k * 1e-3) / 1e12), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(P, 16, 3, device="cuda", generator=g) * 0.25
    y = x + torch.randn(P, 16, 3, device="cuda", generator=g) * 0.05
    B = P // FRAMES
    y4, x4 = y[:B * FRAMES].view(B, FRAMES, 16, 3), x[:B * FRAMES].view(B, FRAMES, 16, 3)
    wj, wp = torch.rand(P, 16, device="cuda", generator=g), torch.rand(P, 1, device="cuda", generator=g)
    zeros = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    pose_bytes = P * 2 * 192
    clip_bytes = B * FRAMES * 2 * 192
    print("%d poses; clips %s; %d rounds of %d calls, median [fastest-slowest]" % (P, tuple(y4.shape), a.rounds, a.calls))
    compare("mpjpe_byjoint (P,16,3)", lambda: ops.pose_column_errors(y, x, col_sums=zeros(16)), lambda: torch_byjoint(y, x),
            pose_bytes, a.rounds, a.calls)
    compare("mpjpe_byjoint (B,243,16,3)", lambda: ops.pose_column_errors(y4, x4, col_sums=zeros(FRAMES * 16)),
            lambda: torch_byjoint(y4, x4), clip_bytes, a.rounds, a.calls)
    compare("mean_velocity_error (P,16,3)", lambda: ops.pose_column_errors(y, x, vel_sum=zeros(1)), lambda: torch_velocity(y, x),
            pose_bytes, a.rounds, a.calls)
    compare("per-joint + velocity, one call", lambda: ops.pose_column_errors(y, x, center=True, col_sums=zeros(16), vel_sum=zeros(1)),
            lambda: (torch_byjoint(y - y[:, :1], x - x[:, :1]), torch_velocity(y - y[:, :1], x - x[:, :1])), pose_bytes,
            a.rounds, a.calls)
    compare("n_mpjpe (B,243,16,3)", lambda: ops.pose_scaled_errors(y4, x4), lambda: torch_n_mpjpe(y4, x4), clip_bytes, a.rounds,
            a.calls)
    compare("weighted_mpjpe, w per joint", lambda: ops.pose_scaled_errors(y, x, w=wj), lambda: torch_weighted(y, x, wj),
            pose_bytes + P * 64, a.rounds, a.calls)
    compare("weighted_mpjpe, w per pose", lambda: ops.pose_scaled_errors(y, x, w=wp), lambda: torch_weighted(y, x, wp),
            pose_bytes + P * 4, a.rounds, a.calls)


if __name__ == "__main__":
    main()
