#!/usr/bin/env python3
"""Generate tests/golden/video_data.npz by RUNNING THE REFERENCE's video real-data path (build container only: the
reference is imported through tests/golden/_ref_import.py, with its root as working directory because
video_mode_random_bl_aug loads ./data_extra/... relative to it).  Re-run with
    python tests/golden/make_golden_video_data.py

Contents (all arrays; 12 synthetic camera-space sequences, lengths 1..17 so that clips are edge-padded on both sides):
  len, x, cam                      the inputs: lengths, the concatenated raw 3D sequences, (12, 16) cameras
  a33_* / a333_*                   video_mode_dataloader_update at architecture 3,3 / 3,3,3 (batch 16) after
                                   np.random.seed(seed): p3 / p2 the post-swap buffers (concatenated), pairs, perm (the
                                   first epoch's permuted pairs), b3d / b2d / bcam the batches of one next_epoch()
                                   concatenated (a333: the first two batches only), bsizes
  aug_*                            GAN_video_ChunkedGenerator over a33's buffers: chunk_length 4, pad 2, causal_shift 1,
                                   augment (flip), seed 5, batch 16
  end_*                            the same without cameras, chunk 1, pad 1, seed 7, endless: num_batches + 3 batches, i.e.
                                   across one epoch boundary; perm / perm2 the two epochs' orders
"""
import copy
import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI                      # noqa: E402
from video_data_util import synth_sequences   # noqa: E402

torch.set_num_threads(1)
LENGTHS = [1, 3, 5, 9, 2, 4, 7, 12, 15, 6, 11, 17]
LEFT, RIGHT = [4, 5, 6, 10, 11, 12], [1, 2, 3, 13, 14, 15]
SEEDS = {"a33": ("3,3", 21), "a333": ("3,3,3", 22)}


def run_epoch(gen, limit=None):
    it = gen.next_epoch()
    if limit is not None:
        it = itertools.islice(it, limit)
    out = [[None if a is None else np.array(a, dtype=np.float32) for a in b] for b in it]
    cat = lambda k: None if out[0][k] is None else np.concatenate([b[k] for b in out])
    return cat(0), cat(1), cat(2), np.array([len(b[2]) for b in out], dtype=np.int32)


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from models_Fk_GAN import video_mode_operate as V

    poses, cams = synth_sequences(LENGTHS, 2024)
    rec = dict(len=np.array(LENGTHS, dtype=np.int32), x=np.concatenate(poses), cam=np.stack(cams))
    buffers = {}
    for tag, (arch, seed) in SEEDS.items():
        data = dict(poses_train=[p.copy() for p in poses], poses_train_2d=[np.zeros((len(p), 16, 2), np.float32) for p in poses],
                    actions_train=["a"] * len(poses), cams_train=[c.copy() for c in cams])
        np.random.seed(seed)
        V.video_mode_dataloader_update(RI.make_args(batch_size=16, architecture=arch), data, "cpu")
        g = data["target_GAN_loader"]
        buffers[tag] = (g.cameras, g.poses_3d, g.poses_2d)
        perm = np.asarray(copy.deepcopy(g).next_pairs()[1], dtype=np.int32)
        bcam, b3, b2, sizes = run_epoch(g, None if tag == "a33" else 2)
        rec.update({tag + "_p3": np.concatenate(g.poses_3d), tag + "_p2": np.concatenate(g.poses_2d),
                    tag + "_pairs": np.array(g.pairs, dtype=np.int32), tag + "_perm": perm, tag + "_b3d": b3,
                    tag + "_b2d": b2, tag + "_bcam": bcam, tag + "_bsizes": sizes, tag + "_seed": np.int32(seed)})

    c, p3, p2 = buffers["a33"]
    g = V.GAN_video_ChunkedGenerator(16, c, p3, p2, chunk_length=4, pad=2, causal_shift=1, shuffle=True, random_seed=5,
                                     augment=True, kps_left=LEFT, kps_right=RIGHT, joints_left=LEFT, joints_right=RIGHT)
    perm = np.asarray(copy.deepcopy(g).next_pairs()[1], dtype=np.int32)
    bcam, b3, b2, sizes = run_epoch(g)
    rec.update(aug_pairs=np.array(g.pairs, dtype=np.int32), aug_perm=perm, aug_b3d=b3, aug_b2d=b2, aug_bcam=bcam,
               aug_bsizes=sizes)

    g = V.GAN_video_ChunkedGenerator(16, None, p3, p2, chunk_length=1, pad=1, shuffle=True, random_seed=7, endless=True,
                                     kps_left=LEFT, kps_right=RIGHT, joints_left=LEFT, joints_right=RIGHT)
    r = copy.deepcopy(g.random)
    perm, perm2 = r.permutation(g.pairs), r.permutation(g.pairs)
    _, b3, b2, sizes = run_epoch(g, g.num_batches + 3)
    rec.update(end_pairs=np.array(g.pairs, dtype=np.int32), end_perm=perm.astype(np.int32), end_perm2=perm2.astype(np.int32),
               end_b3d=b3, end_b2d=b2, end_bsizes=sizes)

    path = os.path.join(HERE, "video_data.npz")
    np.savez_compressed(path, **rec)
    print("wrote video_data.npz %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(rec)))


if __name__ == "__main__":
    main()
