"""Drop-in for R/models_baseline/videopose/model_VideoPose3D.py: the VideoPose networks, one implementation on activations as rows
(batch-major, then time).

    multiFrame_TemporalModelBase   Conv(k0) + BN + ReLU + drop, per further width k [ Conv(k) + BN + ReLU + drop,
                                   x + (Conv(1) + BN + ReLU + drop) ], Conv(1) + bias.  Its two classes, the strided training model
                                   and the dilated evaluation model, are in models_Fk_GAN/mulit_farme_videopose.py (the reference's
                                   place for them), which also describes the tap layout of the layers with k > 1.
    TemporalModelOptimized1f       the posenet of the reference's default run (:163-220, built with every filter width 1 by
                                   R/function_baseline/model_pos_preparation.py:34-40): the strided model at k = 1, where every
                                   layer is Linear + BN + ReLU + drop.  It differs in three things: 'bf16x6' runs in one launch per
                                   product (no autograd_ops.ORDERED6), the input is (B, 16, 2) or (B, 32) and the output
                                   (B, 16, 3) with a zero hip joint in front, and the constructor refuses every width but 1.

The parameters live in nn.Conv1d / nn.BatchNorm1d containers of the reference's names, shapes and creation order: checkpoints load
in both directions, between the classes too, and one seed gives the reference's initial weights.  What runs on the GPU:
  training    (strided classes) autograd_ops.linear / conv_taps (MFMA GEMM, no epilogue) + autograd_ops.bn_act (dhaug_bn_partials /
              dhaug_bn_act_forward and their two backward launches: batch statistics, running buffers, ReLU, Philox dropout and the
              residual in one pass);
  evaluation  (gradients off) BatchNorm folded into the layer in front of it (dhaug_bn_fold scales rows, which commutes with the tap
              permutation) and the GEMM's bias + ReLU epilogue; a block's second layer, whose residual joins AFTER the ReLU (the
              GEMM epilogue adds residuals before it), runs the plain GEMM and dhaug_bn_act_forward with the running statistics
              given.  The folded and packed operands are cached on the module until a weight, a BatchNorm parameter or a running
              buffer changes.
Everything else is a few lines of plain torch: CPU tensors, evaluation mode with gradients on, and the dilated class in training
mode (the reference never trains it).  Causal and dense convolutions are not implemented (the reference's drivers set neither).

The row-layer paths also serve models_baseline/mlp/linear_model.py (LinearModel derives from TemporalModelOptimized1f): a layer may
be an nn.Linear (a 2-D weight) and may have a bias in front of its BatchNorm -- see _bias_before_bn for training, and in evaluation
the fold carries it through the BatchNorm (dhaug_bn_fold_bias).  The VideoPose layers have no bias and take the calls they took."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd_ops as A
from ... import ops
from ...models_Fk_GAN.Fk_generator import default_precision, graph_precision

PRECISIONS = ("bf16", "bf16x3", "bf16x6")


class multiFrame_TemporalModelBase(nn.Module):
    """the network for any odd filter widths, (B, T, J, F) -> (B, T', J_out, 3); a class says how its k-tap layers address frames"""
    STRIDED = None          # True: stride k over non-overlapping frames (the kernels train it); False: dilated over a sequence

    def __init__(self, num_joints_in, in_features, num_joints_out, filter_widths, causal, dropout, channels):
        super().__init__()
        filter_widths = [int(w) for w in filter_widths]
        name = type(self).__name__
        if not filter_widths or any(w < 1 or w % 2 == 0 for w in filter_widths):
            raise ValueError("%s: only odd filter widths are supported, got filter_widths=%r" % (name, filter_widths))
        if causal:
            raise NotImplementedError("%s: causal convolutions are not implemented" % name)
        if channels % 16 and any(w > 1 for w in filter_widths):     # (the tap views of a layer with k > 1 take unpadded bf16 rows)
            raise ValueError("%s: channels must be a multiple of 16, got %d" % (name, channels))
        self.num_joints_in, self.in_features, self.num_joints_out = num_joints_in, in_features, num_joints_out
        self.filter_widths = filter_widths
        self.channels = channels
        self.precision = default_precision()
        C = channels
        # Parameter holders only (their forward is never called), created in the reference's order: state_dict() lists keys in this
        # order and torch's default initialisation draws from the generator in this order.
        self.drop = nn.Dropout(dropout)
        self.pad = [filter_widths[0] // 2]
        self.causal_shift = [0]
        self.expand_bn = nn.BatchNorm1d(C, momentum=0.1)
        self.shrink = nn.Conv1d(C, num_joints_out * 3, 1)
        strided = self.STRIDED
        self.expand_conv = nn.Conv1d(num_joints_in * in_features, C, filter_widths[0], stride=filter_widths[0] if strided else 1,
                                     bias=False)
        convs, bns = [], []
        dilation = filter_widths[0]
        for w in filter_widths[1:]:
            self.pad.append((w - 1) * dilation // 2)
            self.causal_shift.append(0)
            convs.append(nn.Conv1d(C, C, w, stride=w, bias=False) if strided else nn.Conv1d(C, C, w, dilation=dilation, bias=False))
            bns.append(nn.BatchNorm1d(C, momentum=0.1))
            convs.append(nn.Conv1d(C, C, 1, dilation=1, bias=False))
            bns.append(nn.BatchNorm1d(C, momentum=0.1))
            dilation *= w
        self.layers_conv = nn.ModuleList(convs)
        self.layers_bn = nn.ModuleList(bns)
        self._eval_cache = None
        self._stat_epoch = 0            # training forwards so far: the kernels update the running buffers through raw pointers

    # ------------------------------------------------------------------------------------------------ the reference's interface
    def set_bn_momentum(self, momentum):
        for _, bn, _, _, _ in self._layers():
            bn.momentum = momentum

    def receptive_field(self):
        return 1 + 2 * sum(self.pad)

    def total_causal_shift(self):
        frames = self.causal_shift[0]
        dilation = self.filter_widths[0]
        for i in range(1, len(self.filter_widths)):
            frames += self.causal_shift[i] * dilation
            dilation *= self.filter_widths[i]
        return frames

    def _arithmetic(self):
        """the layer arithmetic of .precision: 'f16x3' (a fused-forward mode of the critics, DHAUG_PRECISION=f16x3) has no layer
        kernels with a backward and runs as 'bf16x6', as the critics' autograd path does"""
        return graph_precision(self.precision)

    def _layer_precision(self):
        """what the layer Functions are given: 'bf16x6' runs its NT products with the correction terms accumulated first
        (autograd_ops.ORDERED6: the same operands and kernel in two launches), which the multi-frame networks' short batches need --
        the last block of the video command's network sees B rows, and BatchNorm over few rows amplifies what the GEMM in front of
        it loses"""
        prec = self._arithmetic()
        return A.ORDERED6 if prec == "bf16x6" else prec

    def _layers(self):
        """(conv, bn, adds the block's input, taps, dilation) of every hidden layer.  What the paths below read of a layer: .weight
        ((N, Cin, k), or (N, Cin) of an nn.Linear) and .bias (None in the VideoPose networks; see _bias_before_bn)"""
        out = [(self.expand_conv, self.expand_bn, False, self.filter_widths[0], 1)]
        dilation = self.filter_widths[0]
        for i, w in enumerate(self.filter_widths[1:]):
            out.append((self.layers_conv[2 * i], self.layers_bn[2 * i], False, w, dilation))
            out.append((self.layers_conv[2 * i + 1], self.layers_bn[2 * i + 1], True, 1, 1))
            dilation *= w
        return out

    def _head(self):
        """the output layer, Conv(1) / Linear + bias"""
        return self.shrink

    def _p(self):
        """the dropout rate behind every hidden layer"""
        return float(self.drop.p)

    def _bias_before_bn(self, layer):
        """the bias of a layer whose output goes into a BatchNorm (the nn.Linear layers of models_baseline/mlp), as the layer's GEMM
        adds it.  Under batch statistics it is a constant: BatchNorm subtracts the batch mean, so its gradient is zero in exact
        arithmetic and rounding residue otherwise -- it is added detached (running_mean comes out right by itself, no column sum is
        launched for it, and no optimizer moves it).  Under the running statistics its gradient is real and it stays attached."""
        b = layer.bias
        return b if b is None or not self.training else b.detach()

    def forward(self, x):
        name = type(self).__name__
        if x.dim() != 4 or x.shape[-2] != self.num_joints_in or x.shape[-1] != self.in_features:
            raise ValueError("%s: input must be (B, T, %d, %d), got %s" % (name, self.num_joints_in, self.in_features, tuple(x.shape)))
        B, T = x.shape[0], x.shape[1]
        rf = self.receptive_field()
        if T < rf:
            raise ValueError("%s: %d frames given, the receptive field is %d" % (name, T, rf))
        y = self._run(x.reshape(B, T, self.num_joints_in * self.in_features), (B, self.channels, 1))
        return y.reshape(B, -1, self.num_joints_out, 3)

    def _run(self, x, one_row):
        """the network on (B, T, features): the kernels for a GPU tensor in training mode (strided classes) or in evaluation mode with
        gradients off, plain torch otherwise.  one_row: the input size that the error for a single row of batch statistics names"""
        if not (x.is_cuda and (not torch.is_grad_enabled() if not self.training else self.STRIDED)):
            return self._forward_torch(x)
        name = type(self).__name__
        B, T = x.shape[0], x.shape[1]
        if self._arithmetic() not in PRECISIONS:
            raise ValueError("%s.precision must be one of %s (or 'f16x3', which runs as 'bf16x6'), got %r" % (name, PRECISIONS, self.precision))
        if self.STRIDED and T != self.receptive_field():
            raise ValueError("%s: the strided model takes one receptive field of frames (%d), got %d" % (name, self.receptive_field(), T))
        rows = x.reshape(B * T, -1).float()
        if not self.training:
            return self._forward_eval(rows, B, T)
        if B * T // self.filter_widths[0] == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (one_row,))
        return self._forward_train(rows)

    # ------------------------------------------------------------------------------------------------ plain torch
    def _forward_torch(self, x):
        h = block_in = x.permute(0, 2, 1)                               # (B, features, T)
        for conv, bn, residual, k, dilation in self._layers():
            if not residual:
                block_in = h
            if self.STRIDED:
                z = F.conv1d(h, conv.weight, stride=k)
            else:
                z = F.conv1d(h, conv.weight, dilation=dilation)
            z = F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training, bn.momentum, bn.eps)
            if self.training:
                with torch.no_grad():
                    bn.num_batches_tracked.add_(1)
            h = F.dropout(F.relu(z), self.drop.p, self.training)
            if residual:
                h = res + h
            elif self.STRIDED:
                res = block_in[:, :, k // 2::k]                         # (what a block's SECOND layer adds: its first layer's input)
            else:
                pad = (k - 1) * dilation // 2
                res = block_in[:, :, pad:block_in.shape[2] - pad]
        y = F.conv1d(h, self.shrink.weight, self.shrink.bias)
        return y.permute(0, 2, 1)

    # ------------------------------------------------------------------------------------------------ training (strided class)
    @staticmethod
    def _w2d(conv):
        """the (N, K) matrix of a width-1 convolution (an nn.Linear's weight is one as it is); its packed copies are cached on the
        parameter (autograd_ops._pack)"""
        if conv.weight.dim() == 2:
            return conv.weight
        W = conv.weight.view(conv.weight.shape[0], conv.weight.shape[1])
        W._dhaug_owner = conv.weight
        return W

    def _forward_train(self, h):
        prec = self._layer_precision()
        f32 = prec != "bf16"
        C, p = self.channels, self._p()
        res = None
        layers, head = self._layers(), self._head()
        for conv, bn, residual, k, _ in layers:
            if bn.momentum is None:
                raise NotImplementedError("%s: cumulative moving average (momentum=None) is not implemented" % type(self).__name__)
            if not residual and conv is not layers[0][0]:
                # what the block's second layer adds: rows k r + k // 2 of the block input, read where they lie (k = 1: the block
                # input itself, not a view of it -- no node in the graph, and bf16 rows padded beyond C stay what they are)
                res = h if k == 1 else h.view(h.shape[0] // k, k, C)[:, k // 2]
            if k == 1:
                z = A.linear(h, self._w2d(conv), self._bias_before_bn(conv), None, A.ACT_NONE, 0.0, prec, out_f32=f32)
            else:
                z = A.conv_taps(h, conv.weight, k, prec, out_f32=f32)
            h = A.bn_act(z, bn.weight, bn.bias, res if residual else None,
                         (bn.running_mean, bn.running_var, bn.num_batches_tracked), bn.momentum, bn.eps, p)
        self._stat_epoch += 1
        return A.linear(h, self._w2d(head), head.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)

    # ------------------------------------------------------------------------------------------------ evaluation (both classes)
    def _eval_key(self):
        head = self._head()
        key = [self._arithmetic(), self._stat_epoch, A.pack_key(head.weight), A.tensor_state(head.bias)]
        for conv, bn, _, _, _ in self._layers():
            key += [A.pack_key(conv.weight)] + [A.tensor_state(t) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)] + [bn.eps]
            key.append(None if conv.bias is None else A.tensor_state(conv.bias))      # (folded into the operands like the rest)
        return key

    def _operand(self, W, Cin, k):
        """weight-side operand of A W2d^T in the module's arithmetic, from a fp32 (N, Cin * k) matrix in the Conv1d layout"""
        prec = self._arithmetic()
        N = W.shape[0]
        if prec == "bf16":
            return ops.cast_pad_bf16(W, A.ceil16(Cin)) if k == 1 else ops.conv_taps_pack_bf16(W.view(N, Cin, k), want_nn=False)[0]
        W2d = W if k == 1 else ops.conv_taps_permute_f32(W, N, Cin, k, True)
        return ops.split_bf16(W2d, 1, A.TERMS[prec], A.ceil16(Cin * k))

    def _folded(self):
        key = self._eval_key()
        if self._eval_cache is None or self._eval_cache[0] != key:
            layers = []
            for conv, bn, residual, k, _ in self._layers():
                W = conv.weight.detach().flatten(1)
                Wf, bias, rstd = ops.bn_fold(W, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                                             want_weight=not residual, layer_bias=conv.bias)
                if residual:                    # (the GEMM stays the layer's own, bias included: BatchNorm runs behind it)
                    bias = None if conv.bias is None else conv.bias.detach()
                layers.append((self._operand(W if residual else Wf, conv.weight.shape[1], k), bias, rstd))
            self._eval_cache = (key, layers, self._operand(self._head().weight.detach().flatten(1), self.channels, 1))
        return self._eval_cache[1], self._eval_cache[2]

    def _gemm(self, a, B, N, K, bias, act, out_f32=False):
        """act(a W^T + bias) against the packed operand B: bf16 (M, ceil16 N) in 'bf16' unless out_f32, fp32 (M, N) otherwise"""
        Kp = A.ceil16(K)
        if self._arithmetic() == "bf16":
            ab = a if a.dtype == A.BF16 else ops.cast_pad_bf16(a, Kp)
            cb, cf = ops.gemm_nt(ab, B, N, Kp, bias=bias, act=act, out_bf16=not out_f32, n_pad=A.ceil16(N), out_f32=out_f32)
            return cf if out_f32 else cb
        prec = self._layer_precision()
        return A._nt_split(ops.split_bf16(a, 0, A.TERMS[prec], Kp), B, N, Kp, prec, bias=bias, act=act)

    def _forward_eval(self, h, nseq, t_in):
        layers, shrink = self._folded()
        C, head, first = self.channels, self._head(), self._layers()[0][0]
        bf16 = self._arithmetic() == "bf16"
        res = None
        for (conv, bn, residual, k, dilation), (Bop, bias, rstd) in zip(self._layers(), layers):
            N, Cin = conv.weight.shape[0], conv.weight.shape[1]
            if residual:
                z = self._gemm(h, Bop, N, Cin, bias, A.ACT_NONE)
                yb, yf, _, _ = ops.bn_act_forward(z, N, bn.weight.detach(), bn.bias.detach(), residual=res,
                                                  stats=(bn.running_mean, rstd))
                h = yb if yb is not None else yf
                continue
            block = conv is not first
            if k == 1:                                  # (in either class: h itself, whose bf16 rows may be padded beyond C)
                a = res = h
            elif self.STRIDED:
                if block:
                    res = h.view(h.shape[0] // k, k, C)[:, k // 2]
                a = h.view(h.shape[0] // k, k * Cin)
            else:
                pad = (k - 1) * dilation // 2
                if block:
                    # rows pad ... t_in - pad of each sequence: a view for one sequence (what the evaluation loaders yield)
                    res = h[pad:t_in - pad] if nseq == 1 else h.view(nseq, t_in, C)[:, pad:t_in - pad].reshape(-1, C)
                ab, af = ops.tap_gather(h, nseq, t_in, Cin, k, dilation=dilation, want_bf16=bf16, want_f32=not bf16)
                a = ab if bf16 else af
                t_in -= 2 * pad
            h = self._gemm(a, Bop, N, k * Cin, bias, A.ACT_RELU)
        return self._gemm(h, shrink, head.weight.shape[0], C, head.bias.detach(), A.ACT_NONE, out_f32=True)


class TemporalModelOptimized1f(multiFrame_TemporalModelBase):
    """the single-frame posenet, (B, 16, 2) or (B, 32) -> (B, 16, 3): the strided model with every filter width 1"""
    STRIDED = True

    def __init__(self, num_joints_in, in_features, num_joints_out, filter_widths, causal=False, dropout=0.25, channels=1024):
        filter_widths = list(filter_widths)
        if not filter_widths or any(int(w) != 1 for w in filter_widths):
            raise NotImplementedError("TemporalModelOptimized1f: only filter width 1 (the single-frame posenet) is implemented, got "
                                      "filter_widths=%r; the temporal models are multiFrame_TemporalModelOptimized1f and "
                                      "multiFrame_TemporalModel of models_Fk_GAN.mulit_farme_videopose" % (filter_widths,))
        if causal:
            raise NotImplementedError("TemporalModelOptimized1f: causal convolutions belong to the temporal models, which do not "
                                      "implement them either")
        super().__init__(num_joints_in, in_features, num_joints_out, filter_widths, causal, dropout, channels)

    def _layer_precision(self):
        """plain 'bf16x6', one launch per product: every BatchNorm of this network sees the whole batch"""
        return self._arithmetic()

    def forward(self, x):
        B = x.shape[0]
        width = self.num_joints_in * self.in_features
        if x.dim() not in (2, 3) or x.numel() != B * width:
            raise ValueError("%s: input must be (B, %d, %d) or (B, %d), got %s"
                             % (type(self).__name__, self.num_joints_in, self.in_features, width, tuple(x.shape)))
        y = self._run(x.reshape(B, 1, width), (B, self.channels))
        return F.pad(y, (3, 0)).view(B, self.num_joints_out + 1, 3)          # the hip joint: zeros in front

    def _forward_torch(self, x):
        """(B, 1, features) -> (B, 3 J_out): the arithmetic of the network on rows, which also documents the kernels' paths"""
        h = block_in = x[:, 0]
        for conv, bn, residual, _, _ in self._layers():
            if not residual:
                block_in = h
            z = F.linear(h, conv.weight.flatten(1), self._bias_before_bn(conv))
            z = F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training, bn.momentum, bn.eps)
            if self.training:
                with torch.no_grad():
                    bn.num_batches_tracked.add_(1)
            h = F.dropout(F.relu(z), self._p(), self.training)
            if residual:
                h = block_in + h
        head = self._head()
        return F.linear(h, head.weight.flatten(1), head.bias)
