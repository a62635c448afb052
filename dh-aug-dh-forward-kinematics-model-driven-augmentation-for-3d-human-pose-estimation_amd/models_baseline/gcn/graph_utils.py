"""Drop-in for the part of R/models_baseline/gcn/graph_utils.py the posenet factory uses: the adjacency of a skeleton, numpy only
(the reference builds it with scipy.sparse; the result is a dense (J, J) fp32 tensor either way).  SemGraphConv reads only its
pattern, adj > 0."""
import numpy as np
import torch

# the 16-joint Human3.6M skeleton the reference trains on (Human36mDataset after remove_joints and the shoulder rewiring)
H36M_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 8, 10, 11, 8, 13, 14)


def adj_mx_from_parents(parents):
    """(J, J) fp32: an edge between every joint and its parent, both directions, plus self loops, each row divided by its sum"""
    parents = [int(p) for p in parents]
    n = len(parents)
    adj = np.eye(n, dtype=np.float64)
    for i, p in enumerate(parents):
        if p >= 0:
            if p >= n or p == i:
                raise ValueError("adj_mx_from_parents: joint %d has parent %d in a skeleton of %d joints" % (i, p, n))
            adj[i, p] = adj[p, i] = 1.0
    adj /= adj.sum(1, keepdims=True)
    return torch.tensor(adj, dtype=torch.float)


def adj_mx_from_skeleton(skeleton):
    return adj_mx_from_parents(list(skeleton.parents())[:skeleton.num_joints()])
