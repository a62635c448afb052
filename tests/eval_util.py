"""Shared stubs and case builders of the posenet-evaluation tests, their fixture generator and the timing tool (no data
files and no reference code needed)."""
import numpy as np
import torch

EVAL_JOINTS = [0, 2, 5, 5, 9, 14, 15]          # a subset with a repeated index (np.take counts it twice)
SETS = {"s1000": (1000, 11), "s700": (700, 12)}
BATCH = 256
VIDEO_ARCH = "3,3"
VIDEO_LENGTHS = [40, 7, 25, 3, 60]


def grid(a, bits=12):
    """values on a 2^-bits grid (exact in fp32; keeps the stored fixture small)"""
    return (np.round(np.asarray(a, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(np.float32)


def skeleton(rng, n, spread=0.25):
    """(n, 16, 3) fp32 poses: random joints around a root at depth 3-6 m"""
    x = rng.randn(n, 16, 3) * spread
    x[:, :, 2] += rng.uniform(3, 6, size=(n, 1))
    return grid(x)


def rotations(rng, n):
    q = rng.randn(n, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def metric_cases(seed=2025):
    """name -> (pred, target) fp32 (n, 16, 3), 64-256 poses each"""
    rng = np.random.RandomState(seed)
    out = {}
    x = skeleton(rng, 128)
    out["noisy"] = (grid(x + rng.randn(*x.shape) * 0.04), x)
    x = skeleton(rng, 128)
    R, s, t = rotations(rng, 128), rng.uniform(0.5, 2.0, (128, 1, 1)), rng.randn(128, 1, 3)
    out["similarity"] = ((s * np.matmul(x.astype(np.float64), R) + t).astype(np.float32), x)
    x = skeleton(rng, 128)
    y = x * np.array([-1, 1, 1], np.float32) + rng.randn(*x.shape).astype(np.float32) * 0.02
    out["mirrored"] = (grid(y), x)
    x = skeleton(rng, 128)
    y = x + rng.randn(*x.shape).astype(np.float32) * 0.05
    y[:, :, 2] = 4.0
    out["planar"] = (grid(y), x)
    x = skeleton(rng, 64)
    d = rng.randn(64, 1, 3)
    y = (rng.randn(64, 16, 1) * 0.3) * d + rng.randn(64, 1, 3)
    out["collinear"] = (grid(y), x)
    x = skeleton(rng, 96)
    y = grid(x + rng.randn(*x.shape).astype(np.float32) * 0.04)
    out["millimetres"] = ((y * 1000).astype(np.float32), (x * 1000).astype(np.float32))
    out["kilometres"] = ((y / 1000).astype(np.float32), (x / 1000).astype(np.float32))
    # joints on the PCK thresholds: an offset of exactly 0.150 m, and of 0.005 k m, along one axis; half of the poses with
    # a zero target coordinate there (the difference is then the offset itself)
    x = skeleton(rng, 128)
    x[:64, :, 0] = 0.0
    k = rng.randint(0, 31, size=(128, 16))
    k[:, ::4] = 30
    y = x.copy()
    y[:, :, 0] = x[:, :, 0] + (0.005 * k).astype(np.float32)
    y[:, 5, 1] += np.float32(0.150)
    out["thresholds"] = (y.astype(np.float32), x)
    return out


def zero_spread_case(seed=7):
    """poses 0-3: a prediction with every joint at one point; 4-7: such a target; 8-15 ordinary"""
    rng = np.random.RandomState(seed)
    x = skeleton(rng, 16)
    y = grid(x + rng.randn(*x.shape).astype(np.float32) * 0.03)
    y[:4] = y[:4, :1]
    x[4:8] = x[4:8, :1]
    return y.astype(np.float32), x


def eval_set(n, seed):
    """(targets (n, 16, 3), inputs (n, 16, 2)) fp32: root-relative-ish 3D poses and a perspective projection"""
    rng = np.random.RandomState(seed)
    t = skeleton(rng, n)
    i = grid(t[:, :, :2] / t[:, :, 2:] + rng.randn(n, 16, 2) * 0.01, 14)
    t = (t - t[:, :1]).astype(np.float32)
    return t, i


def posenet_weights(seed=3, hidden=64):
    rng = np.random.RandomState(seed)
    return dict(w1=(rng.randn(hidden, 32) * 0.3).astype(np.float32), b1=(rng.randn(hidden) * 0.1).astype(np.float32),
                w2=(rng.randn(48, hidden) * 0.05).astype(np.float32), b2=(rng.randn(48) * 0.01).astype(np.float32))


class StubPosenet(torch.nn.Module):
    """a two-layer MLP posenet: (N, 32) 2D keypoints -> (N, 48) 3D joints"""

    def __init__(self, w):
        super().__init__()
        self.l1 = torch.nn.Linear(32, w["w1"].shape[0])
        self.l2 = torch.nn.Linear(w["w1"].shape[0], 48)
        with torch.no_grad():
            for lin, a, b in ((self.l1, "w1", "b1"), (self.l2, "w2", "b2")):
                lin.weight.copy_(torch.as_tensor(np.asarray(w[a])))
                lin.bias.copy_(torch.as_tensor(np.asarray(w[b])))

    def forward(self, x):
        return self.l2(torch.relu(self.l1(x)))


def video_weights(frames, seed=4):
    rng = np.random.RandomState(seed)
    return dict(vw=(rng.randn(48, frames * 32) * 0.05).astype(np.float32), vb=(rng.randn(48) * 0.01).astype(np.float32))


class StubVideoPosenet(torch.nn.Module):
    """(B, frames, 16, 2) -> (B, 1, 16, 3): one linear layer over the receptive field"""

    def __init__(self, w):
        super().__init__()
        self.lin = torch.nn.Linear(w["vw"].shape[1], 48)
        with torch.no_grad():
            self.lin.weight.copy_(torch.as_tensor(np.asarray(w["vw"])))
            self.lin.bias.copy_(torch.as_tensor(np.asarray(w["vb"])))

    def forward(self, x):
        return self.lin(x.reshape(x.shape[0], -1)).view(x.shape[0], 1, 16, 3)


def video_sequences(seed=5):
    rng = np.random.RandomState(seed)
    p3 = [skeleton(rng, n) for n in VIDEO_LENGTHS]
    p2 = [grid(p[:, :, :2] / p[:, :, 2:], 14) for p in p3]
    p3 = [(p - p[:, :1]).astype(np.float32) for p in p3]
    return p3, p2


class ReplayGenerator:
    """next_epoch() yields recorded (cam, batch_3d, batch_2d) batches, as the reference's ChunkedGenerator yields them"""

    def __init__(self, b3d, b2d, sizes, device=None):
        o = np.concatenate([[0], np.cumsum(sizes)])
        conv = (lambda a: a) if device is None else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device))
        self.batches = [(None, conv(b3d[o[i]:o[i + 1]]), conv(b2d[o[i]:o[i + 1]])) for i in range(len(sizes))]

    def num_frames(self):
        return sum(b[1].shape[0] for b in self.batches)

    def next_epoch(self):
        for b in self.batches:
            yield b


class Summary:
    def __init__(self, epoch):
        self.epoch = epoch


class Writer:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, name, value, step=None):
        self.scalars.append((name, float(value), step))


def video_args(posenet_name="videopose"):
    import argparse
    return argparse.Namespace(architecture=VIDEO_ARCH, posenet_name=posenet_name)
