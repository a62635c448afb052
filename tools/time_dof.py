"""The DOF angle distributions (dhaug_dof_histogram, dhaug_dof_pair_histogram) against the torch expression on the same GPU, at
rows = 65 536, D = 37 (9.7 MB of angles, already on the device):

  (a) dof_histogram, angles uniform in (-180, 180)      (b) dof_histogram, every angle 12.5 (one LDS counter per slot)
  (c) dof_pair_histogram, one pair, uniform             (d) dof_pair_histogram, one pair, every angle 12.5: all 65 536 adds
  (e) torch: trunc, clamp, slot * 361 + bin, bincount       of the launch go to ONE word (equal bins are not folded per wave)

The variants alternate in one process; a round is `--calls` back-to-back calls between two HIP events, the figure the median of
`--rounds` rounds after a warm-up of all.  (a)-(d) include the wrappers' workspace allocation.  For scale, a
per-element double Python loop over a host tensor (the way the reference builds the table) runs at 1 024 rows, once.  Not a gate: it prints.

    python tools/time_dof.py [--rounds 5] [--calls 50]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import dhaug_amd  # noqa: F401
from dhaug_amd import ops

ROWS, D, BINS = 65536, 37, 361


def torch_histogram(a):
    b = torch.trunc(a).clamp_(-180, 180).long() + 180
    idx = b + torch.arange(D, device=a.device) * BINS
    return torch.bincount(idx.reshape(-1), minlength=D * BINS)


def host_double_loop(rows):
    """one tensor element read, converted and counted at a time, slot by slot: the cost model of a per-element Python loop"""
    table = torch.zeros((rows.shape[1], BINS))
    for slot in range(rows.shape[1]):
        column = rows[:, slot]
        for value in column:
            table[slot, int(value) + 180] += 1
    return table


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(5)
    uniform = torch.rand(ROWS, D, device="cuda", generator=g) * 360 - 180
    equal = torch.full((ROWS, D), 12.5, device="cuda")
    rec = ops.dof_record(D)
    table = torch.zeros(1, BINS, BINS, dtype=torch.int64, device="cuda")
    variants = [("(a) dof_histogram, uniform", lambda: ops.dof_histogram(uniform, rec)),
                ("(b) dof_histogram, all equal", lambda: ops.dof_histogram(equal, rec)),
                ("(c) dof_pair_histogram, uniform", lambda: ops.dof_pair_histogram(uniform, [(8, 3)], table)),
                ("(d) dof_pair_histogram, all equal", lambda: ops.dof_pair_histogram(equal, [(8, 3)], table)),
                ("(e) torch trunc + bincount", lambda: torch_histogram(uniform))]
    for _ in range(3):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            times[name].append(timed(fn, a.calls))
    print("rows %d, D %d; %d rounds of %d calls, median [fastest-slowest]" % (ROWS, D, a.rounds, a.calls))
    for name, _ in variants:
        t = times[name]
        print("%-36s %8.1f us [%.1f-%.1f]" % (name, float(np.median(t)) * 1e3, min(t) * 1e3, max(t) * 1e3), flush=True)
    small = uniform[:1024].cpu()
    t0 = time.perf_counter()
    want = host_double_loop(small)
    dt = time.perf_counter() - t0
    got = torch_histogram(uniform[:1024]).reshape(D, BINS).cpu()
    assert torch.equal(got, want.long())
    print("per-element double loop on the host, 1 024 rows: %.2f s (%.0f us per row)" % (dt, dt / 1024 * 1e6))


if __name__ == "__main__":
    main()
