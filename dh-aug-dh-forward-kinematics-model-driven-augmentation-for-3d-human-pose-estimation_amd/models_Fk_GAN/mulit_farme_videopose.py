"""Drop-in for R/models_Fk_GAN/mulit_farme_videopose.py (the reference's location and spelling): the posenets of the video mode,

    multiFrame_TemporalModelOptimized1f   training: every k-tap convolution has stride k over non-overlapping frames, the input is
                                          one receptive field of frames and the output one frame;
    multiFrame_TemporalModel              evaluation: the same weights as dilated convolutions over a whole sequence.

With activations as rows (batch-major, then time) a k-tap layer is a plain product A W2d^T, W2d[n, j C + c] = W[n, c, j]:
  strided   A is the layer's input itself, viewed (rows / k, k C); the block's residual x[:, :, k // 2 :: k] is row k r + k // 2 of
            the block input, a row-strided view the BatchNorm kernel reads where it lies;
  dilated   row t of A is the concatenation of rows t, t + d, ..., t + (k - 1) d of its sequence (dhaug_tap_gather); the residual is
            rows pad ... T - pad of each sequence.
BatchNorm over (B, C, T') is BatchNorm over the B T' rows.  So the GEMM, BatchNorm, dropout and optimizer kernels are the
single-frame posenet's (models_baseline/videopose/model_VideoPose3D.py); what is added is the tap layout (csrc/dhaug_taps.hip).

The parameters live in nn.Conv1d / nn.BatchNorm1d containers of the reference's names, shapes and creation order: checkpoints load
in both directions, between the two classes too, and one seed gives the reference's initial weights.  What runs where:
  strided class, training mode, GPU    autograd_ops.conv_taps / linear + autograd_ops.bn_act;
  both classes, evaluation mode with   BatchNorm folded into the layer in front of it (dhaug_bn_fold scales rows, which commutes with
  gradients off, GPU                   the tap permutation) and the GEMM's bias + ReLU epilogue; a block's second layer runs the plain
                                       GEMM and dhaug_bn_act_forward with the running statistics and the residual.  The operands are
                                       cached on the module until a weight, a BatchNorm parameter or a running buffer changes;
  everything else                      plain torch (F.conv1d / F.batch_norm / F.dropout): CPU tensors, evaluation mode with gradients
                                       on, and the dilated class in training mode (the reference never trains it).
.precision: 'bf16x6' is the parity mode (its NT products run as autograd_ops.ORDERED6), 'bf16' and 'bf16x3' are throughput modes.
Causal and dense variants are not implemented (the reference's drivers never set either)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import autograd_ops as A
from .. import ops
from .Fk_generator import default_precision, graph_precision

PRECISIONS = ("bf16", "bf16x3", "bf16x6")


def _state(t):
    return (t.data_ptr(), t._version, getattr(t, "_dhaug_epoch", 0))


class multiFrame_TemporalModelBase(nn.Module):
    STRIDED = None          # set by the two classes

    def __init__(self, num_joints_in, in_features, num_joints_out, filter_widths, causal, dropout, channels):
        super().__init__()
        filter_widths = [int(w) for w in filter_widths]
        name = type(self).__name__
        if not filter_widths or any(w < 1 or w % 2 == 0 for w in filter_widths):
            raise ValueError("%s: only odd filter widths are supported, got filter_widths=%r" % (name, filter_widths))
        if causal:
            raise NotImplementedError("%s: causal convolutions are not implemented" % name)
        if channels % 16:
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
        self.expand_bn.momentum = momentum
        for bn in self.layers_bn:
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
        """the layer arithmetic of .precision ('f16x3' runs as 'bf16x6', as on the single-frame class)"""
        return graph_precision(self.precision)

    def _layer_precision(self):
        """what the layer Functions are given: 'bf16x6' runs its NT products with the correction terms accumulated first
        (autograd_ops.ORDERED6: the same operands and kernel in two launches), which this network's short batches need -- the last
        block of the video command's network sees B rows, and BatchNorm over few rows amplifies what the GEMM in front of it loses"""
        prec = self._arithmetic()
        return A.ORDERED6 if prec == "bf16x6" else prec

    def _layers(self):
        """(conv, bn, adds the block's input, taps, dilation) of every hidden layer"""
        out = [(self.expand_conv, self.expand_bn, False, self.filter_widths[0], 1)]
        dilation = self.filter_widths[0]
        for i, w in enumerate(self.filter_widths[1:]):
            out.append((self.layers_conv[2 * i], self.layers_bn[2 * i], False, w, dilation))
            out.append((self.layers_conv[2 * i + 1], self.layers_bn[2 * i + 1], True, 1, 1))
            dilation *= w
        return out

    def forward(self, x):
        name = type(self).__name__
        if x.dim() != 4 or x.shape[-2] != self.num_joints_in or x.shape[-1] != self.in_features:
            raise ValueError("%s: input must be (B, T, %d, %d), got %s" % (name, self.num_joints_in, self.in_features, tuple(x.shape)))
        B, T = x.shape[0], x.shape[1]
        rf = self.receptive_field()
        if T < rf:
            raise ValueError("%s: %d frames given, the receptive field is %d" % (name, T, rf))
        x = x.reshape(B, T, self.num_joints_in * self.in_features)
        kernels = x.is_cuda and (not torch.is_grad_enabled() if not self.training else self.STRIDED)
        if not kernels:
            y = self._forward_torch(x)
        else:
            if self._arithmetic() not in PRECISIONS:
                raise ValueError("%s.precision must be one of %s (or 'f16x3', which runs as 'bf16x6'), got %r"
                                 % (name, PRECISIONS, self.precision))
            if self.STRIDED and T != rf:
                raise ValueError("%s: the strided model takes one receptive field of frames (%d), got %d" % (name, rf, T))
            rows = x.reshape(B * T, -1).float()
            if self.training:
                if B * T // self.filter_widths[0] == 1:
                    raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                                     % ((B, self.channels, 1),))
                y = self._forward_train(rows)
            else:
                y = self._forward_eval(rows, B, T)
        return y.reshape(B, -1, self.num_joints_out, 3)

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
        """the (N, K) matrix of a width-1 convolution; its packed copies are cached on the parameter (autograd_ops._pack)"""
        W = conv.weight.view(conv.weight.shape[0], conv.weight.shape[1])
        W._dhaug_owner = conv.weight
        return W

    def _forward_train(self, h):
        prec = self._layer_precision()
        f32 = prec != "bf16"
        C, p = self.channels, float(self.drop.p)
        res = None
        for conv, bn, residual, k, _ in self._layers():
            if bn.momentum is None:
                raise NotImplementedError("%s: cumulative moving average (momentum=None) is not implemented" % type(self).__name__)
            if residual:
                z = A.linear(h, self._w2d(conv), None, None, A.ACT_NONE, 0.0, prec, out_f32=f32)
            else:
                if conv is not self.expand_conv:
                    res = h.view(h.shape[0] // k, k, C)[:, k // 2]     # rows k r + k // 2 of the block input, read where they lie
                if k == 1:
                    z = A.linear(h, self._w2d(conv), None, None, A.ACT_NONE, 0.0, prec, out_f32=f32)
                else:
                    z = A.conv_taps(h, conv.weight, k, prec, out_f32=f32)
            h = A.bn_act(z, bn.weight, bn.bias, res if residual else None,
                         (bn.running_mean, bn.running_var, bn.num_batches_tracked), bn.momentum, bn.eps, p)
        self._stat_epoch += 1
        return A.linear(h, self._w2d(self.shrink), self.shrink.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)

    # ------------------------------------------------------------------------------------------------ evaluation (both classes)
    def _eval_key(self):
        key = [self._arithmetic(), self._stat_epoch, A.pack_key(self.shrink.weight), _state(self.shrink.bias)]
        for conv, bn, _, _, _ in self._layers():
            key += [A.pack_key(conv.weight), _state(bn.weight), _state(bn.bias), _state(bn.running_mean), _state(bn.running_var), bn.eps]
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
                                             want_weight=not residual)
                layers.append((self._operand(W if residual else Wf, conv.weight.shape[1], k), None if residual else bias, rstd))
            self._eval_cache = (key, layers, self._operand(self.shrink.weight.detach().flatten(1), self.channels, 1))
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
        C = self.channels
        bf16 = self._arithmetic() == "bf16"
        res = None
        for (conv, bn, residual, k, dilation), (Bop, bias, rstd) in zip(self._layers(), layers):
            N, Cin = conv.weight.shape[0], conv.weight.shape[1]
            if residual:
                z = self._gemm(h, Bop, N, Cin, None, A.ACT_NONE)
                yb, yf, _, _ = ops.bn_act_forward(z, N, bn.weight.detach(), bn.bias.detach(), residual=res,
                                                  stats=(bn.running_mean, rstd))
                h = yb if yb is not None else yf
                continue
            block = conv is not self.expand_conv
            if self.STRIDED:
                if block:
                    res = h.view(h.shape[0] // k, k, C)[:, k // 2]
                a = h.view(h.shape[0] // k, k * Cin)
            else:
                pad = (k - 1) * dilation // 2
                if block:
                    # rows pad ... t_in - pad of each sequence: a view for one sequence (what the evaluation loaders yield)
                    res = h[pad:t_in - pad] if nseq == 1 else h.view(nseq, t_in, C)[:, pad:t_in - pad].reshape(-1, C)
                if k == 1:
                    a = h
                else:
                    ab, af = ops.tap_gather(h, nseq, t_in, Cin, k, dilation=dilation, want_bf16=bf16, want_f32=not bf16)
                    a = ab if bf16 else af
                t_in -= 2 * pad
            h = self._gemm(a, Bop, N, k * Cin, bias, A.ACT_RELU)
        return self._gemm(h, shrink, self.shrink.weight.shape[0], C, self.shrink.bias.detach(), A.ACT_NONE, out_f32=True)


class multiFrame_TemporalModel(multiFrame_TemporalModelBase):
    """the dilated model: (B, T >= receptive field, J, F) -> (B, T - receptive field + 1, J_out, 3)"""
    STRIDED = False

    def __init__(self, num_joints_in, in_features, num_joints_out, filter_widths, causal=False, dropout=0.25, channels=1024,
                 dense=False):
        if dense:
            raise NotImplementedError("multiFrame_TemporalModel: dense convolutions are not implemented")
        super().__init__(num_joints_in, in_features, num_joints_out, filter_widths, causal, dropout, channels)


class multiFrame_TemporalModelOptimized1f(multiFrame_TemporalModelBase):
    """the strided model: (B, receptive field, J, F) -> (B, 1, J_out, 3)"""
    STRIDED = True

    def __init__(self, num_joints_in, in_features, num_joints_out, filter_widths, causal=False, dropout=0.25, channels=1024):
        super().__init__(num_joints_in, in_features, num_joints_out, filter_widths, causal, dropout, channels)
