"""Shared pieces of the MLP posenet tests (models_baseline/mlp): the seeded state, a stock-torch container with the reference's
parameter names and an fp64 restatement of the network.  Inputs and the training pairs are posenet_util's.  No reference code;
nothing here imports the package under test."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from posenet_util import make_inputs, train_data, ulp32, load_golden, TRAIN  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posenet_mlp.npz")
GOLDEN_F32 = os.path.join(ROOT, "tests", "golden", "posenet_mlp_f32.npz")         # the reference class's own fp32 run

# ---- records of the fixture ---------------------------------------------------------------------------------------------------
LAYOUTS = ((1024, 2), (1024, 4))
INIT = dict(C=64, stages=2, seed=5)              # init_*: torch.manual_seed + construction + apply(init_weights)
SMALL = dict(C=64, stages=2, seed=21)            # record (a), rows 96 and 40, and record (c)
WIDE = dict(C=1024, stages=2, seed=22)           # record (b), rows 96
ROWS_A, ROWS_B = (96, 40), 96
RAGGED = dict(C=40, stages=1, seed=24)           # no fixture: the smallest shape with ragged tiles, rows 33, against network_ref
ROWS_RAGGED = 33
BIAS_SCALE = 0.25                                # a fold that drops the layer bias is off by ~0.25 * gamma * rstd


def layer_names(stages):
    """(linear, batchnorm) of every hidden layer in forward order"""
    out = [("w1", "batch_norm1")]
    for i in range(stages):
        out += [("linear_stages.%d.w1" % i, "linear_stages.%d.batch_norm1" % i), ("linear_stages.%d.w2" % i, "linear_stages.%d.batch_norm2" % i)]
    return out


def pre_bn_biases(stages):
    return [lin + ".bias" for lin, _ in layer_names(stages)]


def shapes(C, stages):
    """state_dict key -> (shape, dtype) in the reference's order"""
    s = OrderedDict()
    for j, (lin, bn) in enumerate(layer_names(stages)):
        s[lin + ".weight"] = ((C, 32 if j == 0 else C), torch.float32)
        s[lin + ".bias"] = ((C,), torch.float32)
        for k in ("weight", "bias", "running_mean", "running_var"):
            s["%s.%s" % (bn, k)] = ((C,), torch.float32)
        s[bn + ".num_batches_tracked"] = ((), torch.int64)
    s["w2.weight"] = ((45, C), torch.float32)
    s["w2.bias"] = ((45,), torch.float32)
    return s


def seeded_state(C, stages, seed):
    """Linear weights U(+-1/sqrt(fan_in)), every bias and beta U(+-BIAS_SCALE), gamma U(0.5, 1.5), running statistics (0, 1)"""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for k, (shp, dt) in shapes(C, stages).items():
        if k.endswith("num_batches_tracked"):
            v = np.zeros(shp, np.int64)
        elif k.endswith("running_mean"):
            v = np.zeros(shp, np.float32)
        elif k.endswith("running_var"):
            v = np.ones(shp, np.float32)
        elif len(shp) == 2:
            v = ((rs.random_sample(shp) * 2 - 1) / np.sqrt(shp[1])).astype(np.float32)
        elif "batch_norm" in k and k.endswith(".weight"):
            v = (rs.random_sample(shp) + 0.5).astype(np.float32)
        else:
            v = ((rs.random_sample(shp) * 2 - 1) * BIAS_SCALE).astype(np.float32)
        out[k] = torch.from_numpy(v)
    return out


class StockBlock(nn.Module):
    def __init__(self, C, dropout):
        super().__init__()
        self.w1, self.batch_norm1 = nn.Linear(C, C), nn.BatchNorm1d(C)
        self.w2, self.batch_norm2 = nn.Linear(C, C), nn.BatchNorm1d(C)
        self.drop = nn.Dropout(dropout)

    def forward(self, x):
        u = self.drop(torch.relu(self.batch_norm1(self.w1(x))))
        return x + self.drop(torch.relu(self.batch_norm2(self.w2(u))))


class StockMLP(nn.Module):
    """the network from stock nn.Linear / nn.BatchNorm1d / nn.Dropout modules under the reference's parameter names, every bias
    attached (the floor of the parity tests and the other side of the checkpoint round trip)"""

    def __init__(self, C, stages, dropout=0.0):
        super().__init__()
        self.w1, self.batch_norm1 = nn.Linear(32, C), nn.BatchNorm1d(C)
        self.linear_stages = nn.ModuleList([StockBlock(C, dropout) for _ in range(stages)])
        self.w2 = nn.Linear(C, 45)
        self.drop = nn.Dropout(dropout)

    def pre_bn_biases(self):
        return [self.w1.bias] + [b for blk in self.linear_stages for b in (blk.w1.bias, blk.w2.bias)]

    def forward(self, x):
        B = x.shape[0]
        h = self.drop(torch.relu(self.batch_norm1(self.w1(x.reshape(B, 32)))))
        for blk in self.linear_stages:
            h = blk(h)
        y = self.w2(h)
        return torch.cat([torch.zeros_like(y[:, :3]), y], 1).view(B, 16, 3)


def network_ref(state, x, t, eps=1e-5, momentum=0.1):
    """the network in fp64 with matmul, training mode, dropout 0, every bias attached: dict(out, loss, grads {key: tensor},
    buffers {key: tensor}, eval_out (evaluation-mode output with the updated buffers))"""
    P = {k: (v.double().clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
         for k, v in state.items()}
    stages = sum(1 for k in state if k.endswith(".w1.weight"))
    M = x.shape[0]
    buffers = {}

    def run(train):
        h = block_in = x.double().reshape(M, 32)
        for j, (lin, bn) in enumerate(layer_names(stages)):
            residual = j > 0 and j % 2 == 0
            if not residual:
                block_in = h
            z = h @ P[lin + ".weight"].t() + P[lin + ".bias"]
            if train:
                mean, var = z.mean(0), z.var(0, unbiased=False)
                buffers[bn + ".running_mean"] = (1 - momentum) * P[bn + ".running_mean"].double() + momentum * mean.detach()
                buffers[bn + ".running_var"] = (1 - momentum) * P[bn + ".running_var"].double() + momentum * var.detach() * M / (M - 1)
            else:
                mean, var = buffers[bn + ".running_mean"], buffers[bn + ".running_var"]
            h = torch.relu((z - mean) / torch.sqrt(var + eps) * P[bn + ".weight"] + P[bn + ".bias"])
            if residual:
                h = block_in + h
        y = h @ P["w2.weight"].t() + P["w2.bias"]
        return torch.cat([torch.zeros_like(y[:, :3]), y], 1).view(M, 16, 3)

    out = run(True)
    loss = ((out - t.double()) ** 2).mean()
    loss.backward()
    grads = {k: v.grad.detach() for k, v in P.items() if v.dtype.is_floating_point and v.requires_grad}
    with torch.no_grad():
        eval_out = run(False)
    return dict(out=out.detach(), loss=loss.detach(), grads=grads, buffers=buffers, eval_out=eval_out)


def state_of(G, prefix, C, stages):
    """a state_dict recorded under `prefix` as tensors"""
    return OrderedDict((k, torch.from_numpy(np.array(G[prefix + k]))) for k in shapes(C, stages))
