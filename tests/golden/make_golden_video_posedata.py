#!/usr/bin/env python3
"""Generate tests/golden/video_posedata.npz by RUNNING THE REFERENCE's ChunkedGenerator and UnchunkedGenerator
(R/models_Fk_GAN/video_mode_operate.py:193-406; build container only: the reference is imported through
tests/golden/_ref_import.py, nothing of it is copied).  Re-run with
    python tests/golden/make_golden_video_posedata.py

The inputs are a33_p3 / a33_p2 / cam / len of the committed video_data.npz (12 sequences of 1..17 frames), so only outputs are
stored here; every batch is cast to fp32, which is exact (the inputs are fp32).  Contents, per tag of video_posedata_util.CHUNKED:
  <tag>_pairs, <tag>_perm          the pair list and the first epoch's order (shuffle=False: the list itself)
  <tag>_b3d / _b2d / _bcam         the batches of one next_epoch() concatenated; absent where the reference yields None
  <tag>_bsizes                     clips per batch
  end_perm2                        the endless run's second order; its batches are num_batches + 3, across the epoch boundary
and per tag of video_posedata_util.UNCHUNKED (one batch per sequence, (1 or 2, T, 16, C)):
  <tag>_b3d / _b2d                 the batches flattened to frames, (sum of m * T, 16, C), in epoch order
  <tag>_bcam                       (sum of m, 16)
"""
import copy
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI                                              # noqa: E402
from video_posedata_util import CHUNKED, UNCHUNKED, LR, inputs       # noqa: E402


def f32(a):
    return None if a is None else np.array(a, dtype=np.float32)       # a copy: the reference reuses its batch buffers


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    cwd = os.getcwd()
    os.chdir(RI.REF_ROOT)
    from models_Fk_GAN import video_mode_operate as V
    os.chdir(cwd)

    z = np.load(os.path.join(HERE, "video_data.npz"))
    G = {k: z[k] for k in z.files}
    rec = {}
    for tag, (batch_size, kw) in CHUNKED.items():
        cam, p3, p2 = inputs(G, tag)
        g = V.ChunkedGenerator(batch_size, cam, p3, p2, **kw)
        r = copy.deepcopy(g.random)
        order = r.permutation(g.pairs) if g.shuffle else np.array(g.pairs)
        rec[tag + "_pairs"] = np.array(g.pairs, dtype=np.int32)
        rec[tag + "_perm"] = np.asarray(order, dtype=np.int32)
        it = g.next_epoch()
        if g.endless:
            rec[tag + "_perm2"] = np.asarray(r.permutation(g.pairs), dtype=np.int32)
            it = itertools.islice(it, g.num_batches + 3)
        out = [[f32(a) for a in b] for b in it]
        for k, name in enumerate(("_bcam", "_b3d", "_b2d")):
            if out[0][k] is not None:
                rec[tag + name] = np.concatenate([b[k] for b in out])
        rec[tag + "_bsizes"] = np.array([len(b[2]) for b in out], dtype=np.int32)
    for tag, kw in UNCHUNKED.items():
        cam, p3, p2 = inputs(G, tag)
        g = V.UnchunkedGenerator(cam, p3, p2, **kw)
        out = [[f32(a) for a in b] for b in g.next_epoch()]
        rec[tag + "_bcam"] = np.concatenate([b[0] for b in out])
        rec[tag + "_b3d"] = np.concatenate([b[1].reshape(-1, 16, 3) for b in out])
        rec[tag + "_b2d"] = np.concatenate([b[2].reshape(-1, 16, 2) for b in out])

    path = os.path.join(HERE, "video_posedata.npz")
    if os.path.exists(path):
        old = np.load(path)
        same = sorted(old.files) == sorted(rec)
        diff = max([float(np.abs(old[k].astype(np.float64) - rec[k]).max()) for k in rec if k in old.files and old[k].shape == rec[k].shape]
                   + [0.0])
        print("against the committed file: same keys %s, max abs diff %g" % (same, diff))
    np.savez_compressed(path, **rec)
    print("wrote video_posedata.npz %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(rec)))


if __name__ == "__main__":
    main()
