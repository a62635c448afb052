"""Drop-in for R/models_Fk_GAN/mulit_farme_videopose.py (the reference's location and spelling): the posenets of the video mode,

    multiFrame_TemporalModelOptimized1f   training: every k-tap convolution has stride k over non-overlapping frames, the input is
                                          one receptive field of frames and the output one frame;
    multiFrame_TemporalModel              evaluation: the same weights as dilated convolutions over a whole sequence.

Both are multiFrame_TemporalModelBase of models_baseline/videopose/model_VideoPose3D.py (where the reference keeps its
TemporalModelBase), which holds the whole network -- parameters, checkpoints, training, evaluation cache, plain-torch path -- and has
the single-frame posenet as its k = 1 case.  What the layers with k > 1 add is the tap layout (csrc/dhaug_taps.hip): with activations
as rows (batch-major, then time) a k-tap layer is a plain product A W2d^T, W2d[n, j C + c] = W[n, c, j]:
  strided   A is the layer's input itself, viewed (rows / k, k C); the block's residual x[:, :, k // 2 :: k] is row k r + k // 2 of
            the block input, a row-strided view the BatchNorm kernel reads where it lies;
  dilated   row t of A is the concatenation of rows t, t + d, ..., t + (k - 1) d of its sequence (dhaug_tap_gather); the residual is
            rows pad ... T - pad of each sequence.
BatchNorm over (B, C, T') is BatchNorm over the B T' rows.
.precision: 'bf16x6' is the parity mode (its NT products run as autograd_ops.ORDERED6), 'bf16' and 'bf16x3' are throughput modes.
Causal and dense variants are not implemented (the reference's drivers never set either)."""
from ..models_baseline.videopose.model_VideoPose3D import PRECISIONS, multiFrame_TemporalModelBase  # noqa: F401


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
