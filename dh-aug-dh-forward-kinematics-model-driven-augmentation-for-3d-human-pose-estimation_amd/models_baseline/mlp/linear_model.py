"""Drop-in for R/models_baseline/mlp/linear_model.py: the MLP posenet of `--posenet_name mlp` (the "simple yet effective baseline"),
(B, 16, 2) or (B, 32) -> (B, 16, 3) with a zero hip joint in front:

    Linear + BN + ReLU + drop, num_stage x [ x + (Linear + BN + ReLU + drop, Linear + BN + ReLU + drop) ], Linear.

That is the arithmetic of the single-frame VideoPose posenet (models_baseline/videopose/model_VideoPose3D.py: the strided model at
k = 1), and LinearModel runs on that class's paths -- training on autograd_ops.linear + autograd_ops.bn_act, evaluation with
gradients off on folded, cached operands, plain torch for everything else -- under the reference's own parameter names (w1,
batch_norm1, linear_stages.{i}.{w1, batch_norm1, w2, batch_norm2}, w2; nn.Linear / nn.BatchNorm1d holders in the reference's creation
order: checkpoints load in both directions, and torch.manual_seed + construction + .apply(init_weights) on the host gives the
reference's initial state).  Two things differ from the VideoPose class:

  * every hidden nn.Linear has a bias in front of its BatchNorm.  In training mode that bias is a CONSTANT here
    (multiFrame_TemporalModelBase._bias_before_bn): the GEMM epilogue adds it, so running_mean is what nn.BatchNorm1d records, but
    its gradient -- zero in exact arithmetic, since BatchNorm subtracts the batch mean -- is not computed, no column sum is launched
    for it, and it keeps its bits under any optimizer.  The reference in fp64 behaves so (gradients <= 1e-16, biases moving <= 1e-11
    in 12 Adam steps); the reference in fp32 feeds rounding residue of ~1e-7 to Adam, whose g / (sqrt(v) + eps) turns it into a random
    walk of ~1e-3 per 12 steps.  In evaluation mode with gradients on the bias is attached: its gradient is real
    there.
  * in evaluation mode every BatchNorm is folded into its Linear by dhaug_bn_fold_bias, which carries the layer's bias through the
    BatchNorm; the cache of folded operands is keyed on every layer bias as well.

.precision: 'bf16x6' is the parity mode (fp32-grade products, one launch per product: every BatchNorm sees the whole batch);
'bf16' and 'bf16x3' are throughput modes and make no parity claim; 'f16x3' runs as 'bf16x6'."""
import torch.nn as nn

from ...models_Fk_GAN.Fk_generator import default_precision
from ..videopose.model_VideoPose3D import TemporalModelOptimized1f


def init_weights(m):
    """model.apply(init_weights): kaiming_normal_ on every nn.Linear weight (biases and BatchNorm keep their defaults)"""
    if isinstance(m, nn.Linear):
        nn.init.kaiming_normal_(m.weight)


class Linear(nn.Module):
    """one residual block's parameter holders under the reference's names.  LinearModel never calls this forward (it reads the
    holders); called on its own the block is stock torch: x + two of (Linear + BN + ReLU + drop)"""

    def __init__(self, linear_size, p_dropout=0.5):
        super().__init__()
        self.l_size = linear_size
        self.relu = nn.ReLU(inplace=True)
        self.dropout = nn.Dropout(p_dropout)
        self.w1 = nn.Linear(linear_size, linear_size)
        self.batch_norm1 = nn.BatchNorm1d(linear_size)
        self.w2 = nn.Linear(linear_size, linear_size)
        self.batch_norm2 = nn.BatchNorm1d(linear_size)

    def forward(self, x):
        h = x
        for lin, bn in ((self.w1, self.batch_norm1), (self.w2, self.batch_norm2)):
            h = self.dropout(self.relu(bn(lin(h))))
        return x + h


class LinearModel(TemporalModelOptimized1f):
    """the MLP posenet: TemporalModelOptimized1f's paths over nn.Linear holders that carry a bias (see the module docstring)"""

    def __init__(self, input_size, output_size, linear_size=1024, num_stage=2, p_dropout=0.5):
        nn.Module.__init__(self)                # (the VideoPose constructors create that network's holders: none of them here)
        if input_size != 32 or output_size != 45:
            raise ValueError("LinearModel: the posenet maps 16 x 2 inputs to 15 x 3 outputs (input_size 32, output_size 45: the "
                             "forward pass views its input as (B, 32) and its output as (B, 16, 3)), got %r and %r"
                             % (input_size, output_size))
        self.linear_size = linear_size
        self.p_dropout = p_dropout
        self.num_stage = num_stage
        self.input_size = input_size
        self.output_size = output_size
        # holders in the reference's creation order: state_dict() lists keys, and the default initialisation draws, in this order
        self.w1 = nn.Linear(input_size, linear_size)
        self.batch_norm1 = nn.BatchNorm1d(linear_size)
        self.linear_stages = nn.ModuleList([Linear(linear_size, p_dropout) for _ in range(num_stage)])
        self.w2 = nn.Linear(linear_size, output_size)
        self.relu = nn.ReLU(inplace=True)
        self.dropout = nn.Dropout(p_dropout)
        # what the shared paths read
        self.num_joints_in, self.in_features, self.num_joints_out = 16, 2, 15
        self.channels = linear_size
        self.filter_widths = [1] * (num_stage + 1)
        self.pad = [0] * (num_stage + 1)
        self.causal_shift = [0] * (num_stage + 1)
        self.precision = default_precision()
        self._eval_cache = None
        self._stat_epoch = 0

    def _layers(self):
        out = [(self.w1, self.batch_norm1, False, 1, 1)]
        for blk in self.linear_stages:
            out += [(blk.w1, blk.batch_norm1, False, 1, 1), (blk.w2, blk.batch_norm2, True, 1, 1)]
        return out

    def _head(self):
        return self.w2

    def _p(self):
        """one rate for the network: the model's own nn.Dropout (the blocks' are built with the same p_dropout)"""
        return float(self.dropout.p)
