"""Seeded H36M-like synthetic sequences for the video loader's tests, fixture and timing tool (no data files needed)."""
import json
import os

import numpy as np

_CAMS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "dh-aug-dh-forward-kinematics-model-driven-augmentation-for-3d-human-pose-estimation_amd", "common",
                     "h36m_cameras.json")


def h36m_cam9():
    """the four H36M cameras' intrinsics as the reference's 9-vectors: f, c (normalised screen coordinates), k(3), p(2)"""
    out = []
    for c in json.load(open(_CAMS))["intrinsic"]:
        w, h = c["res_w"], c["res_h"]
        f = np.array(c["focal_length"]) / w * 2
        ctr = np.array(c["center"]) / w * 2 - np.array([1, h / w])
        out.append(np.concatenate([f, ctr, c["radial_distortion"], c["tangential_distortion"]]))
    return np.array(out, dtype=np.float32)


def synth_sequences(lengths, seed):
    """camera-space pose sequences (n, 16, 3) fp32: a random skeleton (~0.25 m bones) drifting and turning slowly, root at
    depth 3-6 m; plus one 16-wide camera vector per sequence (H36M intrinsics, a unit quaternion, a translation)"""
    rng = np.random.RandomState(seed)
    cam9 = h36m_cam9()
    poses, cams = [], []
    for n in lengths:
        base = rng.randn(16, 3).astype(np.float32) * 0.25
        base[0] = 0
        t = np.arange(n, dtype=np.float32)[:, None, None]
        wobble = 0.03 * np.sin(0.3 * t + rng.rand(1, 16, 3).astype(np.float32) * 6)
        root = np.array([rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), rng.uniform(3, 6)], dtype=np.float32)
        drift = (rng.randn(3) * 0.01).astype(np.float32) * t[:, :, 0]
        poses.append((base[None] + wobble + root + drift[:, None, :]).astype(np.float32).reshape(n, 16, 3))
        q = rng.randn(4)
        cams.append(np.concatenate([cam9[rng.randint(4)], q / np.linalg.norm(q), rng.randn(3) * 2]).astype(np.float32))
    return poses, cams
