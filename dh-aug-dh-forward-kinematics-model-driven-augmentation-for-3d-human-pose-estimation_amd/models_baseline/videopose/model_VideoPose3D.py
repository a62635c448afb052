"""Drop-in for the posenet of the reference's default run, R/models_baseline/videopose/model_VideoPose3D.py
TemporalModelOptimized1f (:163-220) as R/function_baseline/model_pos_preparation.py:34-40 builds it: every filter width 1, so
every convolution acts on a length-1 sequence and the network is dense,

    Linear(32 -> C, no bias) + BN + ReLU + drop
    stages x [ Linear(C -> C) + BN + ReLU + drop,  x + (Linear(C -> C) + BN + ReLU + drop) ]
    Linear(C -> 45) + bias, a zero hip joint in front.

The parameters live in nn.Conv1d / nn.BatchNorm1d containers of the reference's names, so checkpoints load in both directions.
What runs on the GPU:
  training    autograd_ops.linear (MFMA GEMM, no epilogue) + autograd_ops.bn_act (dhaug_bn_partials / dhaug_bn_act_forward and their
              two backward launches: batch statistics, running buffers, ReLU, Philox dropout and the residual in one pass);
  evaluation  (gradients off) BatchNorm folded into the layer in front of it (dhaug_bn_fold) and the GEMM's bias + ReLU epilogue; a
              block's second layer, whose residual joins AFTER the ReLU (the GEMM epilogue adds residuals before it), runs the plain
              GEMM and dhaug_bn_act_forward with the running statistics given.  The folded and packed operands are cached on the
              module until a weight, a BatchNorm parameter or a running buffer changes.
CPU tensors, and evaluation mode with gradients on, take the same few lines of plain torch (F.linear / F.batch_norm / F.dropout).
Temporal models (a filter width other than 1, causal convolutions) are not implemented."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd_ops as A
from ... import ops
from ...models_Fk_GAN.Fk_generator import default_precision, graph_precision

PRECISIONS = ("bf16", "bf16x3", "bf16x6")


def _state(t):
    return (t.data_ptr(), t._version, getattr(t, "_dhaug_epoch", 0))


class TemporalModelOptimized1f(nn.Module):
    def __init__(self, num_joints_in, in_features, num_joints_out, filter_widths, causal=False, dropout=0.25, channels=1024):
        super().__init__()
        filter_widths = list(filter_widths)
        if not filter_widths or any(int(w) != 1 for w in filter_widths):
            raise NotImplementedError("TemporalModelOptimized1f: only filter width 1 (the single-frame posenet) is implemented, got "
                                      "filter_widths=%r; temporal models are not part of this package yet" % (filter_widths,))
        if causal:
            raise NotImplementedError("TemporalModelOptimized1f: causal convolutions belong to the temporal models, which are not "
                                      "implemented")
        self.num_joints_in, self.in_features, self.num_joints_out = num_joints_in, in_features, num_joints_out
        self.filter_widths = filter_widths
        self.channels = channels
        self.precision = default_precision()
        C, blocks = channels, len(filter_widths) - 1
        # Parameter holders only (their forward is never called).  The order of creation is the one thing taken over from the reference:
        # state_dict() lists keys in this order, and torch's default initialisation draws from the generator in this order, so one
        # seed gives the reference's initial weights.  The dropout probability lives in an nn.Dropout so that .drop.p reads as there.
        self.drop = nn.Dropout(dropout)
        self.expand_bn = nn.BatchNorm1d(C, momentum=0.1)
        self.shrink = nn.Conv1d(C, 3 * num_joints_out, 1)
        self.expand_conv = nn.Conv1d(in_features * num_joints_in, C, 1, bias=False)
        self.layers_conv = nn.ModuleList(nn.Conv1d(C, C, 1, bias=False) for _ in range(2 * blocks))
        self.layers_bn = nn.ModuleList(nn.BatchNorm1d(C, momentum=0.1) for _ in range(2 * blocks))
        self._eval_cache = None
        self._stat_epoch = 0            # training forwards so far: the kernels update the running buffers through raw pointers

    def _arithmetic(self):
        """the layer arithmetic of .precision: 'f16x3' (a fused-forward mode of the critics, DHAUG_PRECISION=f16x3) has no layer
        kernels with a backward and runs as 'bf16x6', as the critics' autograd path does"""
        return graph_precision(self.precision)

    def set_bn_momentum(self, momentum):
        self.expand_bn.momentum = momentum
        for bn in self.layers_bn:
            bn.momentum = momentum

    def receptive_field(self):
        return 1

    def total_causal_shift(self):
        return 0

    def _layers(self):
        """(conv, bn, adds the block's input) of every hidden layer"""
        out = [(self.expand_conv, self.expand_bn, False)]
        for i, (conv, bn) in enumerate(zip(self.layers_conv, self.layers_bn)):
            out.append((conv, bn, i % 2 == 1))
        return out

    def forward(self, x):
        B = x.shape[0]
        width = self.num_joints_in * self.in_features
        if x.dim() not in (2, 3) or x.numel() != B * width:
            raise ValueError("TemporalModelOptimized1f: input must be (B, %d, %d) or (B, %d), got %s"
                             % (self.num_joints_in, self.in_features, width, tuple(x.shape)))
        x = x.reshape(B, width)
        if not x.is_cuda or (not self.training and torch.is_grad_enabled()):
            y = self._forward_torch(x)
        else:
            if self._arithmetic() not in PRECISIONS:
                raise ValueError("TemporalModelOptimized1f.precision must be one of %s (or 'f16x3', which runs as 'bf16x6'), got %r"
                                 % (PRECISIONS, self.precision))
            if self.training and B == 1:
                raise ValueError("Expected more than 1 value per channel when training, got input size %s" % ((B, self.channels),))
            y = self._forward_train(x.float()) if self.training else self._forward_eval(x.float())
        return F.pad(y, (3, 0)).view(B, self.num_joints_out + 1, 3)          # the hip joint: zeros in front

    # ------------------------------------------------------------------------------------------------ plain torch
    def _forward_torch(self, x):
        h = block_in = x
        for conv, bn, residual in self._layers():
            if not residual:
                block_in = h
            z = F.linear(h, conv.weight.flatten(1))
            z = F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training, bn.momentum, bn.eps)
            if self.training:
                with torch.no_grad():
                    bn.num_batches_tracked.add_(1)
            h = F.dropout(F.relu(z), self.drop.p, self.training)
            if residual:
                h = block_in + h
        return F.linear(h, self.shrink.weight.flatten(1), self.shrink.bias)

    # ------------------------------------------------------------------------------------------------ training
    @staticmethod
    def _w2d(conv):
        """the (N, K) matrix of a width-1 convolution; its packed copies are cached on the parameter (autograd_ops._pack)"""
        W = conv.weight.view(conv.weight.shape[0], conv.weight.shape[1])
        W._dhaug_owner = conv.weight
        return W

    def _forward_train(self, x):
        prec = self._arithmetic()
        f32 = prec != "bf16"
        h = block_in = x
        for conv, bn, residual in self._layers():
            if bn.momentum is None:
                raise NotImplementedError("TemporalModelOptimized1f: cumulative moving average (momentum=None) is not implemented")
            if not residual:
                block_in = h
            z = A.linear(h, self._w2d(conv), None, None, A.ACT_NONE, 0.0, prec, out_f32=f32)
            h = A.bn_act(z, bn.weight, bn.bias, block_in if residual else None,
                         (bn.running_mean, bn.running_var, bn.num_batches_tracked), bn.momentum, bn.eps, float(self.drop.p))
        self._stat_epoch += 1
        return A.linear(h, self._w2d(self.shrink), self.shrink.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)

    # ------------------------------------------------------------------------------------------------ evaluation
    def _eval_key(self):
        key = [self._arithmetic(), self._stat_epoch, A.pack_key(self.shrink.weight), _state(self.shrink.bias)]
        for conv, bn, _ in self._layers():
            key += [A.pack_key(conv.weight), _state(bn.weight), _state(bn.bias), _state(bn.running_mean), _state(bn.running_var), bn.eps]
        return key

    def _operand(self, W):
        """weight-side operand of x W^T in the module's arithmetic"""
        Kp = A.ceil16(W.shape[1])
        prec = self._arithmetic()
        return ops.cast_pad_bf16(W, Kp) if prec == "bf16" else ops.split_bf16(W, 1, A.TERMS[prec], Kp)

    def _folded(self):
        key = self._eval_key()
        if self._eval_cache is None or self._eval_cache[0] != key:
            layers = []
            for conv, bn, residual in self._layers():
                W = conv.weight.detach().flatten(1)
                Wf, bias, rstd = ops.bn_fold(W, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                                             want_weight=not residual)
                layers.append((self._operand(W if residual else Wf), None if residual else bias, rstd))
            self._eval_cache = (key, layers, self._operand(self.shrink.weight.detach().flatten(1)))
        return self._eval_cache[1], self._eval_cache[2]

    def _gemm(self, h, B, N, K, bias, act):
        """act(h W^T + bias) against the packed operand B: bf16 (M, ceil16 N) in 'bf16', fp32 (M, N) otherwise"""
        Kp = A.ceil16(K)
        if self._arithmetic() == "bf16":
            hb = h if h.dtype == A.BF16 else ops.cast_pad_bf16(h, Kp)
            return ops.gemm_nt(hb, B, N, Kp, bias=bias, act=act, out_bf16=True, n_pad=A.ceil16(N))[0]
        T = A.TERMS[self._arithmetic()]
        return ops.gemm_nt(ops.split_bf16(h, 0, T, Kp), B, N, T * Kp, bias=bias, act=act, out_f32=True)[1]

    def _forward_eval(self, x):
        layers, shrink = self._folded()
        h = block_in = x
        for (conv, bn, residual), (B, bias, rstd) in zip(self._layers(), layers):
            N, K = conv.weight.shape[0], conv.weight.shape[1]
            if not residual:
                block_in = h
                h = self._gemm(h, B, N, K, bias, A.ACT_RELU)
            else:
                z = self._gemm(h, B, N, K, None, A.ACT_NONE)
                yb, yf, _, _ = ops.bn_act_forward(z, N, bn.weight.detach(), bn.bias.detach(), residual=block_in,
                                                  stats=(bn.running_mean, rstd))
                h = yb if yb is not None else yf
        N, K = self.shrink.weight.shape[0], self.shrink.weight.shape[1]
        if self._arithmetic() == "bf16":
            hb = h if h.dtype == A.BF16 else ops.cast_pad_bf16(h, A.ceil16(K))
            return ops.gemm_nt(hb, shrink, N, A.ceil16(K), bias=self.shrink.bias.detach(), out_f32=True)[1]
        return self._gemm(h, shrink, N, K, self.shrink.bias.detach(), A.ACT_NONE)
