"""Shared pieces of the posenet tests: the seeded state and input builders, a stock-torch container with the reference's parameter
names, fp64 restatements of the network and of BatchNorm + ReLU + dropout (forward and backward, mask given), and the launch-shape
constants of csrc/dhaug_posenet.hip the multi-pass sizes are derived from.  No reference code; nothing here imports the package
under test."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posenet_videopose.npz")
GOLDEN_F32 = os.path.join(ROOT, "tests", "golden", "posenet_videopose_f32.npz")       # the reference class's own fp32 run

# ---- launch shape of the BatchNorm kernels (csrc/dhaug_posenet.hip: kLanesPerRow, kRowsPerPass, DHAUG_BN_MAX_CHUNKS) ------------
LANES_PER_ROW = 8            # x 16 bytes: one 128-byte row segment
ROWS_PER_PASS = 32           # rows a 256-thread workgroup covers per pass
MAX_CHUNKS = 32
VEC = {torch.float32: 4, torch.bfloat16: 8}


def launch_of(M, C, dtype):
    """(column strips, row chunks, rows per chunk) of a BatchNorm launch: the host code's arithmetic restated"""
    sc = LANES_PER_ROW * VEC[dtype]
    strips = -(-((C + 15) // 16 * 16) // sc)
    passes = -(-M // ROWS_PER_PASS)
    want = max(1, min(-(-256 // strips), MAX_CHUNKS, passes))
    rpc = -(-passes // want) * ROWS_PER_PASS
    return strips, -(-M // rpc), rpc


# 64 fp32 columns are 2 strips, so the chunk count is capped by MAX_CHUNKS: with more than 2 * MAX_CHUNKS passes every thread loops
# more than twice over its rows, and the ragged 7 rows leave the last pass partly empty
MULTIPASS = (2 * MAX_CHUNKS * ROWS_PER_PASS + 7, 64)

# ---- records of the fixture ---------------------------------------------------------------------------------------------------
SMALL = dict(C=64, stages=2, seed=11)            # record (a), rows 96 and 40, and record (c)
WIDE = dict(C=1024, stages=4, seed=12)           # record (b), rows 96
ROWS_A, ROWS_B = (96, 40), 96
TRAIN = dict(n=520, batch=96, seed=13, lr=1e-3)  # record (c): five batches of 96 and one of 40, flip on: 12 steps


def shapes(C, stages):
    """state_dict key -> (shape, dtype) in the reference's order"""
    s = OrderedDict()

    def bn(name):
        for k in ("weight", "bias", "running_mean", "running_var"):
            s["%s.%s" % (name, k)] = ((C,), torch.float32)
        s[name + ".num_batches_tracked"] = ((), torch.int64)

    bn("expand_bn")
    s["shrink.weight"] = ((45, C, 1), torch.float32)
    s["shrink.bias"] = ((45,), torch.float32)
    s["expand_conv.weight"] = ((C, 32, 1), torch.float32)
    for i in range(2 * stages):
        s["layers_conv.%d.weight" % i] = ((C, C, 1), torch.float32)
    for i in range(2 * stages):
        bn("layers_bn.%d" % i)
    return s


def seeded_state(C, stages, seed):
    """conv weights U(+-1/sqrt(fan_in)), gamma U(0.5, 1.5), beta and the shrink bias U(+-0.25), running statistics (0, 1)"""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for k, (shp, dt) in shapes(C, stages).items():
        if k.endswith("num_batches_tracked"):
            v = np.zeros(shp, np.int64)
        elif k.endswith("running_mean"):
            v = np.zeros(shp, np.float32)
        elif k.endswith("running_var"):
            v = np.ones(shp, np.float32)
        elif "conv" in k or k == "shrink.weight":
            v = ((rs.random_sample(shp) * 2 - 1) / np.sqrt(shp[1])).astype(np.float32)
        elif k.endswith("bn.weight") or (".weight" in k and "bn" in k):
            v = (rs.random_sample(shp) + 0.5).astype(np.float32)
        else:
            v = ((rs.random_sample(shp) * 2 - 1) * 0.25).astype(np.float32)
        out[k] = torch.from_numpy(v)
    return out


def make_inputs(M, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, 16, 2, generator=g)
    t = 0.3 * torch.randn(M, 16, 3, generator=g)
    t[:, 0] = 0
    return x, t


def train_data():
    """record (c)'s pairs: 3D poses (root anywhere: the loop centres them) and 2D inputs"""
    g = torch.Generator().manual_seed(TRAIN["seed"])
    n = TRAIN["n"]
    p3 = 0.3 * torch.randn(n, 16, 3, generator=g) + torch.randn(n, 1, 3, generator=g)
    p2 = 0.4 * torch.randn(n, 16, 2, generator=g)
    return p3, p2


class StockPosenet(nn.Module):
    """the network from stock nn.Conv1d / nn.BatchNorm1d / nn.Dropout modules under the reference's parameter names (the floor of
    the parity tests and the other side of the checkpoint round trip)"""

    def __init__(self, C, stages, dropout=0.0):
        super().__init__()
        self.expand_bn = nn.BatchNorm1d(C, momentum=0.1)
        self.shrink = nn.Conv1d(C, 45, 1)
        self.expand_conv = nn.Conv1d(32, C, 1, bias=False)
        self.layers_conv = nn.ModuleList([nn.Conv1d(C, C, 1, bias=False) for _ in range(2 * stages)])
        self.layers_bn = nn.ModuleList([nn.BatchNorm1d(C, momentum=0.1) for _ in range(2 * stages)])
        self.drop = nn.Dropout(dropout)

    def forward(self, x):
        B = x.shape[0]
        h = torch.relu(self.expand_bn(self.expand_conv(x.reshape(B, 32, 1))))
        h = self.drop(h)
        for i in range(0, len(self.layers_conv), 2):
            u = self.drop(torch.relu(self.layers_bn[i](self.layers_conv[i](h))))
            h = h + self.drop(torch.relu(self.layers_bn[i + 1](self.layers_conv[i + 1](u))))
        y = self.shrink(h).reshape(B, 45)
        return torch.cat([torch.zeros_like(y[:, :3]), y], 1).view(B, 16, 3)


# ---- fp64 restatements ----------------------------------------------------------------------------------------------------------
def network_ref(state, x, t, eps=1e-5, momentum=0.1):
    """the network in fp64 with matmul, training mode, dropout 0: dict(out, loss, grads {key: tensor}, buffers {key: tensor},
    eval_out (evaluation-mode output with the updated buffers))"""
    P = {k: (v.double().clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
         for k, v in state.items()}
    stages = sum(1 for k in state if k.startswith("layers_conv.")) // 2
    names = [("expand_conv", "expand_bn", False)] + [("layers_conv.%d" % i, "layers_bn.%d" % i, i % 2 == 1) for i in range(2 * stages)]
    M = x.shape[0]
    buffers = {}

    def run(train):
        h = block_in = x.double().reshape(M, 32)
        for conv, bn, residual in names:
            if not residual:
                block_in = h
            z = h @ P[conv + ".weight"][:, :, 0].t()
            if train:
                mean, var = z.mean(0), z.var(0, unbiased=False)
                buffers[bn + ".running_mean"] = (1 - momentum) * P[bn + ".running_mean"].double() + momentum * mean.detach()
                buffers[bn + ".running_var"] = (1 - momentum) * P[bn + ".running_var"].double() + momentum * var.detach() * M / (M - 1)
            else:
                mean, var = buffers[bn + ".running_mean"], buffers[bn + ".running_var"]
            h = torch.relu((z - mean) / torch.sqrt(var + eps) * P[bn + ".weight"] + P[bn + ".bias"])
            if residual:
                h = block_in + h
        y = h @ P["shrink.weight"][:, :, 0].t() + P["shrink.bias"]
        return torch.cat([torch.zeros_like(y[:, :3]), y], 1).view(M, 16, 3)

    out = run(True)
    loss = ((out - t.double()) ** 2).mean()
    loss.backward()
    grads = {k: v.grad.detach() for k, v in P.items() if v.dtype.is_floating_point and v.requires_grad}
    with torch.no_grad():
        eval_out = run(False)
    return dict(out=out.detach(), loss=loss.detach(), grads=grads, buffers=buffers, eval_out=eval_out)


def bn_stats_ref(z):
    """(mean, biased var) per column in fp64"""
    z = z.double()
    return z.mean(0), z.var(0, unbiased=False)


def bn_act_ref(z, mean, rstd, gamma, beta, keep=None, inv_keep=1.0, residual=None):
    """fp64: (y, pre) with y = keep * relu(pre) * inv_keep (+ residual), pre = (z - mean) * rstd * gamma + beta"""
    pre = (z.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()
    y = torch.relu(pre)
    if keep is not None:
        y = y * keep.double() * float(inv_keep)
    if residual is not None:
        y = y + residual.double()
    return y, pre


def bn_act_backward_ref(z, g, mean, rstd, gamma, beta, keep=None, inv_keep=1.0, active=None):
    """fp64 backward for the cotangent g: (dz, dgamma, dbeta, gz).  active: the (pre > 0) decisions to use (the kernel's own, read
    back from its forward output) instead of the fp64 sign, which differs where the pre-activation rounds across zero"""
    z, g, mean, rstd, gamma, beta = (t.double() for t in (z, g, mean, rstd, gamma, beta))
    xh = (z - mean) * rstd
    if active is None:
        active = (xh * gamma + beta) > 0
    gz = g * active.double()
    if keep is not None:
        gz = gz * keep.double() * float(inv_keep)
    M = z.shape[0]
    s1, s2 = gz.sum(0), (gz * xh).sum(0)
    dz = gamma * rstd * (gz - s1 / M - xh * s2 / M)
    return dz, s2, s1, gz


def ulp32(x):
    """the fp32 ulp at |x| (fp64 tensor): 2^(floor(log2 |x|) - 23), the smallest normal's below it"""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def load_golden(path=GOLDEN):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def state_of(G, prefix, C, stages):
    """a state_dict recorded under `prefix` as tensors"""
    return OrderedDict((k, torch.from_numpy(np.array(G[prefix + k]))) for k in shapes(C, stages))
