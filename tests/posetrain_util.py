"""Shared pieces of the posenet-training tests: the stub posenet, the fixture's data, the reference loops' steps restated in
plain torch, a numpy restatement of the fused clip + Adam arithmetic (with two deliberately wrong variants), and a stock-torch
run of the loops.  Nothing here imports the package under test."""
import argparse
import os

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posetrain.npz")

LEFT, RIGHT = [4, 5, 6, 10, 11, 12], [1, 2, 3, 13, 14, 15]
LR = 1e-3
FRAMES = 3                                  # 2D frames per clip of the video loops (the 3D side carries one frame)
LOOPS = ("single", "video", "gan")          # train_posenet, video_mode_train_posenet, GAN_dataSet_video_mode_train_posenet
SINGLE = dict(n=520, batch=96)              # five batches of 96 and one of 40; flip on: 12 steps
VIDEO = dict(n=160, batch=64)               # 64, 64, 32; flip and playback on: 12 steps
# targets of alternate batches are scaled so that the gradient norms lie well below and well above max_norm = 1 (the clips'
# wider first layer gives larger gradients, hence the smaller factor)
SCALES = (0.5, 4.0)
VIDEO_SCALES = (0.25, 4.0)


class StubPosenet(nn.Module):
    """Linear(32 F -> 64, no bias) -> BatchNorm1d -> ReLU -> residual ReLU(Linear(64 -> 64)) -> Linear(64 -> 45); the hip joint is
    padded with zeros.  No dropout; no parameter with an identically zero gradient (no bias in front of the BatchNorm).
    frames = 0: the single-frame loop, output (n, 16, 3); frames = F: a clip of F frames in, the output (n, 1, 16, 3)."""

    def __init__(self, frames=0, width=64):
        super().__init__()
        self.frames = frames
        self.a = nn.Linear(32 * max(frames, 1), width, bias=False)
        self.bn = nn.BatchNorm1d(width)
        self.b = nn.Linear(width, width)
        self.c = nn.Linear(width, 45)

    def forward(self, x):
        x = x.reshape(x.shape[0], -1)
        y = torch.relu(self.bn(self.a(x)))
        y = y + torch.relu(self.b(y))
        y = self.c(y)
        y = torch.cat([torch.zeros_like(y[:, :3]), y], 1)
        return y.view(-1, 1, 16, 3) if self.frames else y.view(-1, 16, 3)


def make_model(loop):
    torch.manual_seed(0)
    return StubPosenet(0 if loop == "single" else FRAMES)


def loop_args():
    return argparse.Namespace(flip_pos_model_input=True, GAN_video_playback_input=True)


def make_data():
    """the fixture's inputs: single-frame pairs and clips; the targets of alternate batches scaled by SCALES"""
    g = torch.Generator().manual_seed(3)
    n, B = SINGLE["n"], SINGLE["batch"]
    t3 = torch.randn(n, 16, 3, generator=g) * 3.0 + torch.randn(n, 1, 3, generator=g) * 2
    i2 = torch.randn(n, 16, 2, generator=g) * 0.4
    t3 = t3 * torch.tensor(SCALES)[(torch.arange(n) // B) % 2].view(n, 1, 1)
    n, B = VIDEO["n"], VIDEO["batch"]
    v3 = torch.randn(n, 1, 16, 3, generator=g) * 3.0 + torch.randn(n, 1, 1, 3, generator=g) * 2
    v2 = torch.randn(n, FRAMES, 16, 2, generator=g) * 0.4
    v3 = v3 * torch.tensor(VIDEO_SCALES)[(torch.arange(n) // B) % 2].view(n, 1, 1, 1)
    return dict(s_t3d=t3.numpy(), s_i2d=i2.numpy(), v_b3d=v3.numpy(), v_b2d=v2.numpy())


def batches_of(G, loop, to=lambda a: torch.from_numpy(np.ascontiguousarray(a))):
    """[(3D, 2D)] per batch, through `to` (host tensors by default)"""
    key3, key2, cfg = ("s_t3d", "s_i2d", SINGLE) if loop == "single" else ("v_b3d", "v_b2d", VIDEO)
    return [(to(G[key3][i:i + cfg["batch"]]), to(G[key2][i:i + cfg["batch"]])) for i in range(0, cfg["n"], cfg["batch"])]


class EpochLoader:
    """the interface video_mode_train_posenet reads: num_batches and next_epoch() -> (cam, batch_3d, batch_2d)"""

    def __init__(self, batches):
        self.batches, self.num_batches = batches, len(batches)

    def next_epoch(self):
        for b3, b2 in self.batches:
            yield None, b3, b2


def loader_of(loop, batches):
    """what each of the three loops iterates"""
    if loop == "single":
        return [(b3, b2, ["a"] * len(b3), torch.zeros(len(b3), 9)) for b3, b2 in batches]
    if loop == "video":
        return EpochLoader(batches)
    return [(torch.zeros(len(b3), 9), b3, b2) for b3, b2 in batches]


def flip(x):
    x = x.clone()
    x[..., 0] *= -1
    x[..., LEFT + RIGHT, :] = x[..., RIGHT + LEFT, :]
    return x


def steps_of_batch(loop, b3, b2, use_flip=True, playback=True):
    """(input, target) of every optimizer step the reference takes on one batch, in its order; fp32 tensors on b3's device"""
    b3, b2 = b3.float(), b2.float()
    n = b3.shape[0]
    if loop == "single":
        t = b3 - b3[:, :1, :]
        out = [(b2, t)]
        if use_flip:
            out.append((flip(b2).view(n, -1), flip(t)))
        return out
    if loop == "gan":
        b3 = b3.contiguous().view(-1, 1, 16, 3)
    t = b3 - b3[:, :, :1, :]
    out = [(b2, t)]
    if playback:
        out.append((torch.flip(b2.view(n, -1, 16, 2), dims=[1]), t))
    if use_flip:
        f2, ft = flip(b2), flip(t)
        out.append((f2, ft))
        if playback:
            out.append((torch.flip(f2.view(n, -1, 16, 2), dims=[1]), ft))
    return out


def stock_loop(model, loop, batches, optimizer, criterion, use_flip=True, playback=True):
    """the reference's sequence of calls with stock torch pieces (criterion, clip_grad_norm_, a torch.optim optimizer) on
    whatever device the model and the batches are: returns the per-step losses and norms as device tensors (no host read)"""
    torch.set_grad_enabled(True)
    model.train()
    losses, norms = [], []
    for b3, b2 in batches:
        if b3.shape[0] == 1:
            break
        for inp, tgt in steps_of_batch(loop, b3, b2, use_flip, playback):
            out = model(inp)
            optimizer.zero_grad()
            loss = criterion(out, tgt)
            loss.backward()
            norms.append(nn.utils.clip_grad_norm_(model.parameters(), max_norm=1).detach())
            optimizer.step()
            losses.append(loss.detach())
    return torch.stack(losses), torch.stack(norms)


def restated_loop(model, loop, batches, variant="fused", lr=LR, use_flip=True, playback=True):
    """The arithmetic of dhaug_pose_mse + dhaug_grad_sumsq + dhaug_adam_clip_step restated on the CPU, driving `model` in place:
    grad = 2 (p - t) / numel, the flat fp32 gradient, ONE global fp64 sum of squares, norm rounded to fp32,
    coef = min(1, 1 / (norm + 1e-6)) in fp32, Adam on the flat vectors.  Returns (losses, norms).
    variant "noclamp": coef is not clamped to 1; "pertensor": every tensor is clipped by its own norm -- both wrong on purpose."""
    f32 = np.float32
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    m, v, step = np.zeros(n, f32), np.zeros(n, f32), 0
    b1, b2c, eps = f32(0.9), f32(0.999), f32(1e-8)
    losses, norms = [], []
    model.train()

    def coef_of(g):
        nrm = f32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        c = f32(1.0) / (nrm + f32(1e-6))
        return nrm, (c if variant == "noclamp" else min(f32(1.0), c))

    for b3, b2 in batches:
        if b3.shape[0] == 1:
            break
        for inp, tgt in steps_of_batch(loop, b3, b2, use_flip, playback):
            model.zero_grad()
            out = model(inp)
            d = (out - tgt).detach()
            losses.append(float(f32((d.double() ** 2).mean().item())))
            out.backward(d * f32(2.0 / d.numel()))
            g = np.concatenate([p.grad.reshape(-1).numpy() for p in params]).astype(f32)
            nrm, coef = coef_of(g)
            norms.append(float(nrm))
            if variant == "pertensor":
                off = 0
                for p in params:
                    k = p.numel()
                    g[off:off + k] *= coef_of(g[off:off + k])[1]
                    off += k
            else:
                g = g * coef
            step += 1
            m[:] = m + (g - m) * (f32(1) - b1)
            v[:] = v * b2c + g * g * (f32(1) - b2c)
            bc1, bc2s = f32(1.0 - 0.9 ** step), f32(np.sqrt(1.0 - 0.999 ** step))
            upd = (f32(lr) / bc1) * (m / (np.sqrt(v) / bc2s + eps))
            off = 0
            with torch.no_grad():
                for p in params:
                    k = p.numel()
                    p -= torch.from_numpy(upd[off:off + k]).view(p.shape)
                    off += k
    return np.array(losses), np.array(norms)


def state_arrays(model):
    """float tensors of the state_dict (parameters and BatchNorm statistics) as numpy"""
    return {k: t.detach().cpu().numpy().copy() for k, t in model.state_dict().items() if t.dtype.is_floating_point}


def max_state_diff(model, G, loop):
    """largest absolute difference of any parameter / buffer to the fixture's state after the loop"""
    return max(float(np.abs(a - G["%s_final_%s" % (loop, k)]).max()) for k, a in state_arrays(model).items())


def load_initial(model, G, loop):
    sd = model.state_dict()
    for k in sd:
        sd[k] = torch.from_numpy(np.array(G["%s_init_%s" % (loop, k)]))
    model.load_state_dict(sd)
    return model


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
