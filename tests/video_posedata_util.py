"""Shared pieces of the posenet data loaders' tests and fixture (ChunkedGenerator / UnchunkedGenerator): the recorded
configurations, their inputs out of tests/golden/video_data.npz, the launch shapes the multi-pass sizes are derived from, and an
independent torch restatement of the two-window gather.  Nothing here imports the package under test."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEFT, RIGHT = [4, 5, 6, 10, 11, 12], [1, 2, 3, 13, 14, 15]
LR = dict(kps_left=LEFT, kps_right=RIGHT, joints_left=LEFT, joints_right=RIGHT)
FLIP_PERM = list(range(16))
for _l, _r in zip(LEFT, RIGHT):
    FLIP_PERM[_l], FLIP_PERM[_r] = _r, _l

# tag -> (batch_size, constructor keywords) of the recorded ChunkedGenerator runs
CHUNKED = {
    "c33": (16, dict(chunk_length=1, pad=4, causal_shift=0, augment=False, **LR)),
    "aug": (16, dict(chunk_length=4, pad=2, causal_shift=1, augment=True, random_seed=5, **LR)),
    "c333": (13, dict(chunk_length=1, pad=13, causal_shift=0, augment=False, **LR)),        # 92 clips: the last batch holds one
    "neg": (16, dict(chunk_length=3, pad=2, causal_shift=-2, augment=True, random_seed=9, **LR)),
    "val": (16, dict(chunk_length=1, pad=4, shuffle=False, **LR)),                          # the validation form (:476-511)
    "end": (16, dict(chunk_length=1, pad=1, random_seed=7, endless=True, **LR)),            # no cameras, no 3D
}
# tag -> constructor keywords of the recorded UnchunkedGenerator runs
UNCHUNKED = {
    "u4": dict(pad=4, causal_shift=0, augment=True, **LR),
    "u13": dict(pad=13, causal_shift=13, augment=False, **LR),
    "uneg": dict(pad=4, causal_shift=-4, augment=True, **LR),
}


def load(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    return {k: z[k] for k in z.files}


def split(a, lengths):
    return np.split(a, np.cumsum(lengths)[:-1])


def inputs(G, tag):
    """(cameras, poses_3d, poses_2d) lists of a configuration, from video_data.npz's a33 buffers"""
    L = G["len"]
    p3, p2 = split(G["a33_p3"], L), split(G["a33_p2"], L)
    if tag == "end":
        return None, None, p2
    return list(G["cam"]), p3, p2


def chunked(V, G, tag):
    batch_size, kw = CHUNKED[tag]
    return V.ChunkedGenerator(batch_size, *inputs(G, tag), **kw)


def unchunked(V, G, tag):
    return V.UnchunkedGenerator(*inputs(G, tag), **UNCHUNKED[tag])


# ---- launch shapes of csrc/dhaug_clip.hip that the multi-pass size is derived from.  A changed constant in the source is a size to
# revisit here.
GATHER_BLOCK = 256                   # clip_gather_launch: hipLaunchKernelGGL(clip_gather_kernel, ..., dim3(256), ...)  (:213)
GATHER_GRID_CAP = 256 * 16           # clip_gather_launch: if (blocks > 256 * 16) blocks = 256 * 16                     (:212)
PAIR_BLOCK = 64                      # constexpr int kClipPairBlock = 64                                                (:98)
PAIR_GRID_CAP = 2048                 # constexpr int kClipPairMaxGrid = 2048                                            (:99)
QUADS_PER_PASS = GATHER_GRID_CAP * GATHER_BLOCK         # 1 048 576 16-byte quads (12 per 3D frame, 8 per 2D frame)
POSE_FRAMES_PER_PASS = PAIR_GRID_CAP * PAIR_BLOCK       # 131 072 pose-frames

# the real shape of the box: B = 1024 clips of one 3D frame and 243 2D frames
MULTI_B, MULTI_R = 1024, 243
MULTI_GATHER_PASSES = -(-(MULTI_B * (12 + MULTI_R * 8)) // QUADS_PER_PASS)          # 2
MULTI_PAIR_PASSES = -(-(MULTI_B * (1 + MULTI_R)) // POSE_FRAMES_PER_PASS)           # 2
assert MULTI_GATHER_PASSES >= 2 and MULTI_PAIR_PASSES >= 2


def expected_windows(seq3d, seq2d, off, ln, rec, frames3, shift3, frames2, shift2, perm):
    """(out3d, out2d) by torch.index_select over clamped frame indices: computed here, independently of the kernels.  perm: a
    (16,) index tensor, the flip's joint permutation"""
    import torch
    rec = rec.long()
    out = []
    for s, C, frames, shift in ((seq3d, 3, frames3, shift3), (seq2d, 2, frames2, shift2)):
        f = torch.arange(frames, device=rec.device)
        t = (rec[:, 1:2] - shift + f).clamp(min=0)
        t = torch.minimum(t, ln[rec[:, 0]].long().unsqueeze(1) - 1) + off[rec[:, 0]].unsqueeze(1)
        x = torch.index_select(s, 0, t.reshape(-1)).reshape(-1, frames, 16, C)
        fl = torch.index_select(x, 2, perm)
        fl[..., 0] = -fl[..., 0]
        out.append(torch.where(rec[:, 3].bool().view(-1, 1, 1, 1), fl, x))
    return out


def expected_pairs(p3, p2, perm, flip, playback):
    """ops.pair_batch's dict in plain torch expressions (the reference's: centring, flip, torch.flip over the frames)"""
    import torch

    def fl(x):
        y = torch.index_select(x, 2, perm)
        y[..., 0] = -y[..., 0]
        return y

    out = dict(tgt=p3 - p3[:, :, :1, :], inp=p2)
    if flip:
        out.update(tgt_flip=fl(out["tgt"]), inp_flip=fl(p2))
    if playback:
        out.update(inp_back=torch.flip(p2, dims=[1]))
        if flip:
            out.update(inp_flip_back=torch.flip(out["inp_flip"], dims=[1]))
    return out
