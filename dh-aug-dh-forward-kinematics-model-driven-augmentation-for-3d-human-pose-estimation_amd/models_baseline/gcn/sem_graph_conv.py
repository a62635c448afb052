"""Drop-in for R/models_baseline/gcn/sem_graph_conv.py SemGraphConv: the parameters of one semantic graph convolution under the
reference's names, and its arithmetic in plain torch.  With A = softmax over each row of (e scattered into the pattern adj > 0,
-9e15 elsewhere),

    out[b,i,:] = A[i,i] (x W[0])[b,i,:] + sum_{j != i} A[i,j] (x W[1])[b,j,:] + bias.

SemGCN runs the same layer on the GPU as one GEMM against Wcat = [W[0]^T ; W[1]^T] and one dhaug_graph_mix launch."""
import math

import numpy as np
import torch
import torch.nn as nn

NEG = -9e15            # the reference's fill outside the pattern: exp(NEG - max) is exactly 0 in fp32 and fp64


def pattern_of(adj):
    """(rows, cols) of adj > 0 in row-major order, as Python lists: the order of the elements of e"""
    m = np.asarray(adj.detach().cpu().numpy() if torch.is_tensor(adj) else adj) > 0
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("SemGraphConv: adj must be a square matrix, got shape %s" % (m.shape,))
    r, c = np.nonzero(m)
    return r.tolist(), c.tolist()


_SCATTER_INDEX = {}


def _scatter_index(rows, cols, joints, device):
    """the pattern's flat positions as a device tensor, uploaded once per (pattern, device): an upload per call is a host
    synchronisation, which a training step captured as a hipGraph may not contain"""
    key = (tuple(rows), tuple(cols), joints, str(device))
    if key not in _SCATTER_INDEX:
        _SCATTER_INDEX[key] = torch.as_tensor([r * joints + c for r, c in zip(rows, cols)], dtype=torch.long, device=device)
    return _SCATTER_INDEX[key]


def softmax_adjacency(e, rows, cols, joints):
    """e (L, nnz) -> (L, J, J): one scatter and one softmax for L layers"""
    flat = e.new_full((e.shape[0], joints * joints), NEG)
    idx = _scatter_index(rows, cols, joints, e.device)
    return torch.softmax(flat.index_copy(1, idx, e).view(-1, joints, joints), dim=2)


class SemGraphConv(nn.Module):
    def __init__(self, in_features, out_features, adj, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        # the order of creation and of the random draws is the reference's: W, e, bias
        self.W = nn.Parameter(torch.zeros(size=(2, in_features, out_features), dtype=torch.float))
        nn.init.xavier_uniform_(self.W.data, gain=1.414)
        self.adj = adj                                  # a plain attribute, not part of the state
        self.rows, self.cols = pattern_of(adj)
        self.joints = len(adj)
        self.e = nn.Parameter(torch.ones(1, len(self.rows), dtype=torch.float))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_features, dtype=torch.float))
            stdv = 1.0 / math.sqrt(out_features)
            self.bias.data.uniform_(-stdv, stdv)
        else:
            self.register_parameter("bias", None)

    def adjacency(self):
        return softmax_adjacency(self.e, self.rows, self.cols, self.joints)[0]

    def mix(self, x, A):
        """the layer for x (B, J, in) and a given adjacency A (J, J)"""
        h0, h1 = torch.matmul(x, self.W[0]), torch.matmul(x, self.W[1])
        d = torch.diagonal(A)
        out = d.view(1, -1, 1) * h0 + torch.matmul(A - torch.diag(d), h1)
        return out if self.bias is None else out + self.bias.view(1, 1, -1)

    def forward(self, x):
        return self.mix(x, self.adjacency())

    def __repr__(self):
        return "%s (%d -> %d)" % (self.__class__.__name__, self.in_features, self.out_features)
