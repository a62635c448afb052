"""Drop-in for the SemGCN posenet, R/models_baseline/gcn/sem_gcn.py SemGCN as R/function_baseline/model_pos_preparation.py builds it
(`--posenet_name gcn`: SemGCN(adj, 128, num_layers=stages, p_dropout=dropout, nodes_group=None)):

    SemGraphConv(2 -> C) + BN + ReLU + drop
    num_layers x [ SemGraphConv(C -> C) + BN + ReLU + drop,  x + (SemGraphConv(C -> C) + BN + ReLU + drop) ]
    SemGraphConv(C -> 3)

on (B, 16, 2) inputs; BatchNorm runs per channel over the B x 16 (pose, joint) rows.  The parameters live in containers of the
reference's names (gconv_input.0.gconv.W ... gconv_output.bias), so checkpoints load in both directions, and are created in the
reference's order, so one seed gives the reference's initial weights.  What runs on the GPU, with activations as (16 B, C) rows:
  training    per layer autograd_ops.linear against Wcat = [W[0]^T ; W[1]^T] (one GEMM for h0 and h1), autograd_ops.graph_mix
              (dhaug_graph_mix; backward: its adjoint, dhaug_graph_adj_grad and a column sum) and autograd_ops.bn_act (batch
              statistics, ReLU, Philox dropout and a block's residual in one pass).  The adjacencies of all layers come from ONE
              scatter + softmax of the stacked e (torch ops: e's gradient is autograd's).
  evaluation  (gradients off) the same three launches per layer, BatchNorm in its given-statistics mode; the adjacencies, the
              running rstd and Wcat are cached on the module until a parameter or a running buffer changes.
CPU tensors, and evaluation mode with gradients on, take a few lines of plain torch.  The reference's non-local layers
(nodes_group) are not implemented: its factory always passes None, and its non-local block is commented out."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd_ops as A
from ... import ops
from ...models_Fk_GAN.Fk_generator import default_precision, graph_precision
from .sem_graph_conv import SemGraphConv, softmax_adjacency

PRECISIONS = ("bf16", "bf16x3", "bf16x6")
JOINTS = 16              # the joints dhaug_graph_mix mixes


class _GraphConv(nn.Module):
    """parameter holder: .gconv, .bn (and the dropout probability, read as .dropout.p)"""

    def __init__(self, adj, input_dim, output_dim, p_dropout=None):
        super().__init__()
        self.gconv = SemGraphConv(input_dim, output_dim, adj)
        self.bn = nn.BatchNorm1d(output_dim)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(p_dropout) if p_dropout is not None else None


class _ResGraphConv(nn.Module):
    def __init__(self, adj, input_dim, output_dim, hid_dim, p_dropout):
        super().__init__()
        self.gconv1 = _GraphConv(adj, input_dim, hid_dim, p_dropout)
        self.gconv2 = _GraphConv(adj, hid_dim, output_dim, p_dropout)


class SemGCN(nn.Module):
    def __init__(self, adj, hid_dim, coords_dim=(2, 3), num_layers=4, nodes_group=None, p_dropout=None):
        super().__init__()
        if nodes_group is not None:
            raise NotImplementedError("SemGCN: nodes_group (the non-local layers) is not implemented; the reference's factory passes None")
        if hid_dim < 16 or hid_dim % 16:
            raise ValueError("SemGCN: hid_dim must be a multiple of 16 (the GEMM operands' padding), got %r" % (hid_dim,))
        if len(adj) != JOINTS:
            raise ValueError("SemGCN: the adjacency must be %d x %d (the joint-mix kernel's skeleton), got %d rows" % (JOINTS, JOINTS, len(adj)))
        self.hid_dim, self.coords_dim, self.num_layers = hid_dim, tuple(coords_dim), num_layers
        self.precision = default_precision()
        # modules in the reference's order: gconv_input, gconv_layers, gconv_output
        self.gconv_input = nn.Sequential(_GraphConv(adj, coords_dim[0], hid_dim, p_dropout=p_dropout))
        self.gconv_layers = nn.Sequential(*[_ResGraphConv(adj, hid_dim, hid_dim, hid_dim, p_dropout=p_dropout) for _ in range(num_layers)])
        self.gconv_output = SemGraphConv(hid_dim, coords_dim[1], adj)
        self._const = {}                # device -> the pattern as an int32 (nnz, 2) tensor
        self._eval_cache = None
        self._stat_epoch = 0            # training forwards so far: the kernels update the running buffers through raw pointers
        self.eval_builds = 0            # times the evaluation cache was (re)built

    def _arithmetic(self):
        """'f16x3' (a fused-forward mode of the critics) has no layer kernels with a backward and runs as 'bf16x6'"""
        return graph_precision(self.precision)

    def _layers(self):
        """(SemGraphConv, BatchNorm1d, dropout p, adds the block's input) of every hidden layer"""
        p = lambda gc: float(gc.dropout.p) if gc.dropout is not None else 0.0
        first = self.gconv_input[0]
        out = [(first.gconv, first.bn, p(first), False)]
        for blk in self.gconv_layers:
            out.append((blk.gconv1.gconv, blk.gconv1.bn, p(blk.gconv1), False))
            out.append((blk.gconv2.gconv, blk.gconv2.bn, p(blk.gconv2), True))
        return out

    def _convs(self):
        return [l[0] for l in self._layers()] + [self.gconv_output]

    def _adjacencies(self):
        """(layers, 16, 16): every layer's softmax adjacency from one scatter and one softmax of the stacked e"""
        g = self.gconv_output
        return softmax_adjacency(torch.cat([c.e for c in self._convs()], 0), g.rows, g.cols, JOINTS)

    def _pairs(self, device):
        if device not in self._const:
            g = self.gconv_output
            self._const[device] = torch.tensor(list(zip(g.rows, g.cols)), dtype=torch.int32, device=device).reshape(-1, 2)
        return self._const[device]

    def forward(self, x):
        B = x.shape[0]
        cin = self.coords_dim[0]
        if x.dim() not in (2, 3) or x.numel() != B * JOINTS * cin:
            raise ValueError("SemGCN: input must be (B, %d, %d) or (B, %d), got %s" % (JOINTS, cin, JOINTS * cin, tuple(x.shape)))
        x = x.reshape(B, JOINTS, cin)
        for _, bn, _, _ in self._layers():
            if bn.momentum is None:
                raise NotImplementedError("SemGCN: cumulative moving average (momentum=None) is not implemented")
        if not x.is_cuda or (not self.training and torch.is_grad_enabled()):
            return self._forward_torch(x)
        if self._arithmetic() not in PRECISIONS:
            raise ValueError("SemGCN.precision must be one of %s (or 'f16x3', which runs as 'bf16x6'), got %r" % (PRECISIONS, self.precision))
        rows = x.float().reshape(B * JOINTS, cin)
        y = self._forward_train(rows) if self.training else self._forward_eval(rows)
        return y.view(B, JOINTS, self.coords_dim[1])

    # ------------------------------------------------------------------------------------------------ plain torch
    def _forward_torch(self, x):
        B = x.shape[0]
        adj = self._adjacencies().unbind(0)
        h = block_in = x.to(self.gconv_output.W.dtype)
        for k, (conv, bn, p, residual) in enumerate(self._layers()):
            if not residual:
                block_in = h
            z = conv.mix(h, adj[k]).reshape(B * JOINTS, -1)
            z = F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training, bn.momentum, bn.eps)
            if self.training:
                with torch.no_grad():
                    bn.num_batches_tracked.add_(1)
            h = F.dropout(F.relu(z), p, self.training).view(B, JOINTS, -1)
            if residual:
                h = block_in + h
        return self.gconv_output.mix(h, adj[-1])

    # ------------------------------------------------------------------------------------------------ training
    def _forward_train(self, x):
        prec = self._arithmetic()
        f32 = prec != "bf16"
        adj = self._adjacencies().unbind(0)
        pairs = self._pairs(x.device)
        h = block_in = x
        for k, (conv, bn, p, residual) in enumerate(self._layers()):
            if not residual:
                block_in = h
            H = A.linear(h, A.graph_wcat(conv.W), None, None, A.ACT_NONE, 0.0, prec, out_f32=f32)
            z = A.graph_mix(H, adj[k], conv.bias, pairs, conv.out_features)
            h = A.bn_act(z, bn.weight, bn.bias, block_in if residual else None,
                         (bn.running_mean, bn.running_var, bn.num_batches_tracked), bn.momentum, bn.eps, p)
        self._stat_epoch += 1
        conv = self.gconv_output
        H = A.linear(h, A.graph_wcat(conv.W), None, None, A.ACT_NONE, 0.0, prec, out_f32=True)
        return A.graph_mix(H, adj[-1], conv.bias, pairs, conv.out_features)

    # ------------------------------------------------------------------------------------------------ evaluation
    def _eval_key(self):
        key = [self._arithmetic(), self._stat_epoch]
        for conv in self._convs():
            key += [A.pack_key(conv.W), A.tensor_state(conv.e), None if conv.bias is None else A.tensor_state(conv.bias)]
        for _, bn, _, _ in self._layers():
            key += [A.tensor_state(t) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)] + [bn.eps]
        return key

    def _eval_state(self):
        """(adjacencies, [Wcat], [running rstd]) of the current state"""
        key = self._eval_key()
        if self._eval_cache is None or self._eval_cache[0] != key:
            adj = self._adjacencies().detach().unbind(0)
            wcat = [A.graph_wcat(conv.W.detach()) for conv in self._convs()]
            for w, conv in zip(wcat, self._convs()):
                w._dhaug_owner = conv.W                  # the packed operands live on the parameter (autograd_ops._pack)
            rstd = [ops.bn_fold(None, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, want_weight=False)[2]
                    for _, bn, _, _ in self._layers()]
            self._eval_cache = (key, adj, wcat, rstd)
            self.eval_builds += 1
        return self._eval_cache[1:]

    def _forward_eval(self, x):
        prec = self._arithmetic()
        f32 = prec != "bf16"
        adj, wcat, rstd = self._eval_state()
        h = block_in = x
        for k, (conv, bn, _, residual) in enumerate(self._layers()):
            if not residual:
                block_in = h
            H = A.linear(h, wcat[k], None, None, A.ACT_NONE, 0.0, prec, out_f32=f32)
            z = ops.graph_mix(H, adj[k], None if conv.bias is None else conv.bias.detach(), conv.out_features)
            yb, yf, _, _ = ops.bn_act_forward(z, conv.out_features, bn.weight.detach(), bn.bias.detach(),
                                              residual=block_in if residual else None, stats=(bn.running_mean, rstd[k]))
            h = yb if yb is not None else yf
        conv = self.gconv_output
        H = A.linear(h, wcat[-1], None, None, A.ACT_NONE, 0.0, prec, out_f32=True)
        return ops.graph_mix(H, adj[-1], None if conv.bias is None else conv.bias.detach(), conv.out_features)
