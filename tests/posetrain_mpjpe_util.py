"""Shared pieces of the MPJPE posenet-training tests, on top of posetrain_util: the gain of the stub's last layer, the
reference's mpjpe expression restated in torch, and a CPU restatement of dhaug_pose_mpjpe's arithmetic driving
posetrain_util.restated_loop's clip + Adam.  Nothing here imports the package under test."""
import os

import numpy as np
import torch
import torch.nn as nn

import posetrain_util as PU

GOLDEN = os.path.join(PU.ROOT, "tests", "golden", "posetrain_mpjpe.npz")
LOOPS = ("video", "gan")                    # video_mode_train_posenet, GAN_dataSet_video_mode_train_posenet
# The MPJPE gradient is a unit vector per joint over the joint count: its size does not follow the targets' scale, so
# posetrain_util's scaled targets cannot move the gradient norm across max_norm = 1.  With the stub as posetrain_util builds it
# all 12 norms lie in 0.31 .. 0.48; the last layer's weight times GAIN puts four of them at 0.78 .. 0.81 and eight at
# 1.10 .. 1.27.
GAIN = 3.2


def make_model(loop):
    model = PU.make_model(loop)
    with torch.no_grad():
        model.c.weight.mul_(GAIN)
    return model


class LearnableHip(nn.Module):
    """The stub with a learnable offset, initialised to zero, on the hip joint it pads with zeros.  Against root-centred targets
    the hip's distance is exactly 0, so a criterion with the zero subgradient leaves the offset at exactly 0 (Adam with a zero
    gradient and zero moments does not move) and the stub inside follows the fixture; a criterion that divides by the distance
    sends 0 / 0 = NaN into the offset's gradient, through the gradient norm into the clip coefficient, and from there into
    every parameter.  (On the stub alone that NaN lands on the constant padding and reaches no parameter.)"""

    def __init__(self, stub):
        super().__init__()
        self.stub = stub
        self.hip = nn.Parameter(torch.zeros(3))

    def forward(self, x):
        y = self.stub(x)
        return y + torch.cat([self.hip.view(1, 3), torch.zeros(15, 3)])


def torch_mpjpe(predicted, target):
    """the reference's criterion, mean(norm(predicted - target, dim=-1)), in stock torch"""
    return torch.mean(torch.norm(predicted - target, dim=len(target.shape) - 1))


def mpjpe_grad(out, tgt, guard=True):
    """dhaug_pose_mpjpe's arithmetic on the CPU: fp64 differences and distances, grad = fl32(d / (e * joints)), exactly 0 at
    distance 0 (guard=False: the division as it stands, NaN there -- wrong on purpose).  Returns (loss fl32, grad fp32)."""
    d = (out.detach().double() - tgt.double())
    e = torch.sqrt((d * d).sum(-1, keepdim=True))
    joints = e.numel()
    g = d / (e * joints)
    if guard:
        g = torch.where(e == 0, torch.zeros_like(g), g)
    return float(np.float32((e.sum() / joints).item())), g.float()


def restated_mpjpe_loop(model, loop, batches, guard=True, lr=PU.LR):
    """posetrain_util.restated_loop with the MSE gradient replaced by mpjpe_grad (that function forms its gradient inside, so its
    clip + Adam lines are repeated here statement for statement): the flat fp32 gradient, ONE global fp64 sum of
    squares, norm rounded to fp32, coef = min(1, 1 / (norm + 1e-6)) in fp32, Adam on the flat vectors.  Returns (losses, norms)."""
    f32 = np.float32
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    m, v, step = np.zeros(n, f32), np.zeros(n, f32), 0
    b1, b2c, eps = f32(0.9), f32(0.999), f32(1e-8)
    losses, norms = [], []
    model.train()
    for b3, b2 in batches:
        if b3.shape[0] == 1:
            break
        for inp, tgt in PU.steps_of_batch(loop, b3, b2):
            model.zero_grad()
            out = model(inp)
            loss, grad = mpjpe_grad(out, tgt, guard)
            losses.append(loss)
            out.backward(grad)
            g = np.concatenate([p.grad.reshape(-1).numpy() for p in params]).astype(f32)
            nrm = f32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
            norms.append(float(nrm))
            c = f32(1.0) / (nrm + f32(1e-6))
            g = g * (f32(1.0) if c > 1 else c)                      # torch.clamp(c, max=1.0), the kernel's: a NaN stays a NaN
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


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
