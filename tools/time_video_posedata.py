"""The posenet's real-clip loader (models_Fk_GAN/video_mode_operate.ChunkedGenerator) on H36M-sized synthetic data: 600 sequences
of 150-400 frames, B = 1024, chunk_length 1, at 27 and 243 frames per clip, flip and playback on (four training inputs per batch).
Milliseconds per batch of what one iteration of video_mode_train_posenet reads, three ways, alternating in one process:

  (a) fused       next_epoch_pairs(True, True): one dhaug_clip_pair_batch launch per batch
  (b) two-launch  next_epoch() + ops.pair_batch: dhaug_clip_gather_windows, then dhaug_pair_batch
  (c) host        the same batches staged as host float64 numpy (what the reference's ChunkedGenerator yields; its own Python loop
                  that BUILDS them is not in this figure) through _upload_batch + ops.pair_batch

A warm-up pass first; every figure is a host clock around a final synchronise over --batches batches ((c): --host-batches, a
float64 batch at 243 frames is 64 MB), --reps times; median and min..max per path, and the bytes each path moves, from shapes.
Acceptance: the median of (a) is not above the median of (b) by more than the spread (max - min) of (b)'s repetitions.

    python tools/time_video_posedata.py [--frames 27 243] [--reps 5] [--batches 40] [--host-batches 6]
The kernels' own times: the same script under `rocprofv3 --kernel-trace --stats -- python tools/time_video_posedata.py --reps 1`."""
import argparse
import itertools
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
from dhaug_amd.models_Fk_GAN import video_mode_operate as VO

LEFT, RIGHT = VO.JOINTS_LEFT, VO.JOINTS_RIGHT
B = 1024


def ms(t0):
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def sequences(seed=0):
    """resident synthetic sequences: the values do not matter to a gather, the lengths do"""
    lengths = np.random.RandomState(seed).randint(150, 401, 600)
    T = int(lengths.sum())
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (lengths, torch.randn(600, 16, device="cuda", generator=gen), torch.randn(T, 16, 3, device="cuda", generator=gen),
            torch.randn(T, 16, 2, device="cuda", generator=gen))


def run(R, reps, nb, nh):
    lengths, cams, seq3d, seq2d = sequences()
    g = VO.ChunkedGenerator._from_device(B, cams, seq3d, seq2d, lengths, 1, pad=(R - 1) // 2, shuffle=True, augment=False,
                                         kps_left=LEFT, kps_right=RIGHT, joints_left=LEFT, joints_right=RIGHT)
    nb = min(nb, g.num_batches - 1)                       # full batches only
    host = [(b3.cpu().numpy().astype(np.float64), b2.cpu().numpy().astype(np.float64))
            for _, b3, b2 in itertools.islice(g.next_epoch(), nh)]
    dev = torch.device("cuda")

    def fused():
        for _ in itertools.islice(g.next_epoch_pairs(True, True), nb):
            pass
        return nb

    def two():
        for _, b3, b2 in itertools.islice(g.next_epoch(), nb):
            ops.pair_batch(b3, b2, flip=True, playback=True)
        return nb

    def staged():
        for b3, b2 in host:
            ops.pair_batch(VO._upload_batch(b3, dev), VO._upload_batch(b2, dev), flip=True, playback=True)
        return len(host)

    paths = (("(a) fused", fused), ("(b) two-launch", two), ("(c) host float64", staged))
    for _, f in paths:                                    # warm-up: allocator, code objects, pinned staging
        f()
    res = {name: [] for name, _ in paths}
    for _ in range(reps):
        for name, f in paths:                             # (every pass starts with the epoch's shuffle + record upload)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = f()
            res[name].append(ms(t0) / n)
    v3, v2 = B * 48 * 4 / 1e6, B * R * 32 * 4 / 1e6       # MB of one batch's 3D / 2D member in fp32
    moved = {"(a) fused": (v3 + v2) + (2 * v3 + 4 * v2),                              # read the source frames, write six outputs
             "(b) two-launch": 2 * (v3 + v2) + (v3 + v2) + (2 * v3 + 4 * v2),         # + the gathered batch written and read back
             "(c) host float64": (v3 + v2) + (v3 + v2) + (2 * v3 + 4 * v2)}           # H2D copy, then pair_batch (+ 2x that on the host)
    print("R = %d, B = %d, %d batches per pass ((c): %d), %d repetitions; a batch's 2D member is %.1f MB"
          % (R, B, nb, len(host), reps, v2))
    for name, _ in paths:
        t = res[name]
        print("  %-17s %8.4f ms per batch (median; %.4f .. %.4f)  %7.1f MB of device traffic per batch"
              % (name, np.median(t), min(t), max(t), moved[name]))
    a, b = res["(a) fused"], res["(b) two-launch"]
    spread = max(b) - min(b)
    print("  fused - two-launch (medians) %+.4f ms; spread of (b) %.4f ms: %s"
          % (np.median(a) - np.median(b), spread, "accepted" if np.median(a) - np.median(b) <= spread else "NOT accepted"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[27, 243])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--host-batches", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for R in a.frames:
        run(R, max(a.reps, 1), a.batches, a.host_batches)


if __name__ == "__main__":
    main()
