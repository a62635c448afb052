"""Drop-in for the PoseFormer posenet, R/models_baseline/poseformer/model_poseformer.py PoseTransformer as
R/function_baseline/model_pos_preparation.py builds it (`--posenet_name mulit_farme_poseformer`: PoseTransformer(num_frame =
receptive field, num_joints=16, in_chans=2, embed_dim_ratio=32, depth=4, num_heads=8, mlp_ratio=2., qkv_bias=True, qk_scale=None,
drop_path_rate=0.1 for training, 0 for testing)):

    a spatial transformer over the joints of every frame   (sequences of num_joints tokens, width embed_dim_ratio),
    a temporal transformer over the frames of every clip   (sequences of num_frame tokens, width embed_dim_ratio * num_joints),
    a learned weighted mean over the frames, LayerNorm + Linear.

Input anything that views as (-1, num_frame, num_joints, 2), output (b, 1, num_joints, 3).  The parameters live in holders of the
reference's names (Spatial_pos_embed, Temporal_pos_embed, Spatial_patch_to_embedding, Spatial_blocks.{i}.{norm1, attn.qkv, attn.proj,
norm2, mlp.fc1, mlp.fc2}, blocks.{i}..., Spatial_norm, Temporal_norm, weighted_mean, head.0, head.1) created in the reference's
order: checkpoints load in both directions and one seed gives the reference's initial state.  No timm, no einops.

What runs on the GPU, activations as rows (sequence-major, then token), the residual stream fp32 in every mode:
  training    the dense layers (patch embedding, qkv, proj, fc1, fc2, head) on autograd_ops.linear; between them autograd_ops.layer_norm
              (dhaug_layernorm_*), autograd_ops.attention (dhaug_attn_*: q, k and v read in place from the qkv GEMM's output, the result
              written as the proj GEMM's operand) and autograd_ops.gelu (dhaug_gelu_*).  Plain torch: the two position-embedding adds,
              the drop-path masks and their scaling, the weighted mean over the frames, views.  A block without drop path adds its
              residual in the proj / fc2 GEMM epilogue.
  evaluation  (gradients off) the same kernels through ops, nothing saved, both residual adds in the GEMM epilogues.
CPU tensors, and evaluation mode with gradients on, take plain torch (_forward_torch).

THE KEY BIAS.  Softmax does not change when a constant is added to every score of a row, and the k third of a qkv bias adds
q_i . b_k to every score of row i: the output does not depend on that third and its true gradient is exactly zero.  The reference in
fp64 behaves so (gradient <= 3.5e-18, the third moving <= 1.4e-13 in 12 Adam steps); in fp32 the gradient is rounding residue of
about 1e-9, which Adam, dividing by the residue's own size, turns into a drift of up to 1.3e-4 over the same 12 steps.  As with the
MLP posenet's biases in front of a BatchNorm, training on the GPU hands the qkv GEMM the bias with its k third
DETACHED: that third's .grad is exact zeros and it keeps its bits under any optimizer; the q and v thirds are ordinary.

DropPath is this package's own: in training a per-sample Bernoulli(keep) mask divided by keep, drawn from the device generator
(torch.manual_seed reproduces a run; PoseTransformer.drop_path_masks draws a forward's masks in its order); the identity in evaluation
or at rate 0.  Rates follow linspace(0, drop_path_rate, depth), shared by spatial and temporal block i.  drop_rate / attn_drop_rate > 0
are not implemented (the reference's factory never sets them).

.precision: 'bf16x6' is the parity mode; 'bf16' (tensors handed to a GEMM are bf16) and 'bf16x3' are throughput modes and make no
parity claim; 'f16x3' runs as 'bf16x6'."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib
from ... import autograd_ops as A
from ... import ops
from ...models_Fk_GAN.Fk_generator import default_precision, graph_precision

PRECISIONS = ("bf16", "bf16x3", "bf16x6")


def _drop_mask(n, keep, device):
    """n Bernoulli(keep) draws from `device`'s generator, as fp32 0 / 1"""
    return torch.empty(n, dtype=torch.float32, device=device).bernoulli_(keep)


class DropPath(nn.Module):
    """stochastic depth per sample: x * mask / keep in training, the identity in evaluation or at rate 0"""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if not self.training or self.drop_prob == 0.0:
            return x
        keep = 1.0 - self.drop_prob
        mask = _drop_mask(x.shape[0], keep, x.device).to(x.dtype) / keep
        return x * mask.view((-1,) + (1,) * (x.dim() - 1))

    def extra_repr(self):
        return "drop_prob=%g" % self.drop_prob


class Mlp(nn.Module):
    """parameter holders fc1, fc2; called on its own it is stock torch"""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if drop > 0.0:
            raise NotImplementedError("Mlp: dropout inside the transformer is not implemented")
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Attention(nn.Module):
    """parameter holders qkv, proj; called on its own it is stock torch with explicit softmax attention"""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        if attn_drop > 0.0 or proj_drop > 0.0:
            raise NotImplementedError("Attention: dropout inside the transformer is not implemented")
        if dim % num_heads:
            raise ValueError("Attention: dim %d is no multiple of num_heads %d" % (dim, num_heads))
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = qk_scale or self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        p = torch.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * self.scale, dim=-1)
        return self.proj((p @ qkv[2]).transpose(1, 2).reshape(B, N, C))

    def train_bias(self):
        """the qkv bias as training on the GPU sees it: the k third detached (see the module docstring)"""
        b = self.qkv.bias
        if b is None:
            return None
        C = b.numel() // 3
        return torch.cat([b[:C], b[C:2 * C].detach(), b[2 * C:]])


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def rate(self):
        return self.drop_path.drop_prob if isinstance(self.drop_path, DropPath) else 0.0

    def forward(self, x, masks=(None, None)):
        """stock torch on (sequences, tokens, dim); masks: this block's two drop-path masks (0 / 1 per sequence) or None"""
        keep = 1.0 - self.rate()
        for branch, m in ((lambda t: self.attn(self.norm1(t)), masks[0]), (lambda t: self.mlp(self.norm2(t)), masks[1])):
            y = branch(x)
            x = x + (y if m is None else y * (m.to(y.dtype) / keep).view(-1, 1, 1))
        return x


class _LayerNorm(nn.LayerNorm):
    """nn.LayerNorm at the network's eps = 1e-6 (the reference's partial(nn.LayerNorm, eps=1e-6))"""

    def __init__(self, dim):
        super().__init__(dim, eps=1e-6)


class PoseTransformer(nn.Module):
    def __init__(self, num_frame=9, num_joints=17, in_chans=2, embed_dim_ratio=32, depth=4, num_heads=8, mlp_ratio=2., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2, norm_layer=None):
        super().__init__()
        if drop_rate > 0.0 or attn_drop_rate > 0.0:
            raise NotImplementedError("PoseTransformer: drop_rate / attn_drop_rate > 0 (dropout inside the transformer) is not "
                                      "implemented; the reference's factory never sets them")
        if in_chans != 2:
            raise ValueError("PoseTransformer: the forward pass views its input as (-1, num_frame, num_joints, 2): in_chans must be 2")
        embed_dim = embed_dim_ratio * num_joints
        for what, dim in (("embed_dim_ratio", embed_dim_ratio), ("int(embed_dim_ratio * mlp_ratio)", int(embed_dim_ratio * mlp_ratio)),
                          ("int(embed_dim * mlp_ratio)", int(embed_dim * mlp_ratio))):
            if dim < 16 or dim % 16:
                raise ValueError("PoseTransformer: %s must be a multiple of 16 (a bf16 GEMM operand then has no pad columns), got %d"
                                 % (what, dim))
        if embed_dim > _lib.LAYERNORM_MAX_COLS:
            raise ValueError("PoseTransformer: embed_dim_ratio * num_joints = %d is above the LayerNorm kernel's %d columns "
                             "(DHAUG_LAYERNORM_MAX_COLS)" % (embed_dim, _lib.LAYERNORM_MAX_COLS))
        if embed_dim_ratio % num_heads:
            raise ValueError("PoseTransformer: embed_dim_ratio %d is no multiple of num_heads %d" % (embed_dim_ratio, num_heads))
        for what, hd in (("spatial", embed_dim_ratio // num_heads), ("temporal", embed_dim // num_heads)):
            if hd % 4 or not 4 <= hd <= _lib.ATTN_MAX_HEAD_DIM:
                raise ValueError("PoseTransformer: the %s head width %d is outside the attention kernel's range: a multiple of 4 from 4 "
                                 "to %d (DHAUG_ATTN_MAX_HEAD_DIM)" % (what, hd, _lib.ATTN_MAX_HEAD_DIM))
        for what, n in (("num_joints", num_joints), ("num_frame", num_frame)):
            if not 1 <= n <= _lib.ATTN_MAX_TOKENS:
                raise ValueError("PoseTransformer: %s = %d is outside the attention kernel's 1 to %d tokens (DHAUG_ATTN_MAX_TOKENS)"
                                 % (what, n, _lib.ATTN_MAX_TOKENS))
        norm_layer = norm_layer or _LayerNorm
        out_dim = num_joints * 3
        # holders in the reference's creation order: state_dict() lists keys, and the default initialisation draws, in this order
        self.Spatial_patch_to_embedding = nn.Linear(in_chans, embed_dim_ratio)
        self.Spatial_pos_embed = nn.Parameter(torch.zeros(1, num_joints, embed_dim_ratio))
        self.Temporal_pos_embed = nn.Parameter(torch.zeros(1, num_frame, embed_dim))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.Spatial_blocks = nn.ModuleList([
            Block(dim=embed_dim_ratio, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer) for i in range(depth)])
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer) for i in range(depth)])
        self.Spatial_norm = norm_layer(embed_dim_ratio)
        self.Temporal_norm = norm_layer(embed_dim)
        self.weighted_mean = nn.Conv1d(in_channels=num_frame, out_channels=1, kernel_size=1)
        self.head = nn.Sequential(nn.LayerNorm(embed_dim), nn.Linear(embed_dim, out_dim))
        self.num_joints = num_joints
        self.num_frame = num_frame
        self.embed_dim_ratio = embed_dim_ratio
        self.embed_dim = embed_dim
        self.precision = default_precision()

    def _arithmetic(self):
        """'f16x3' (a fused-forward mode of the critics) has no layer kernels with a backward and runs as 'bf16x6'"""
        return graph_precision(self.precision)

    def receptive_field(self):
        return self.num_frame

    # ------------------------------------------------------------------------------------------------ drop path
    def drop_path_masks(self, b, device):
        """the masks of one training forward over b clips, drawn from `device`'s generator in the forward's order: per spatial block,
        then per temporal block, (attention branch, MLP branch); a spatial mask has b * num_frame entries (one per frame), a temporal
        one b; None where the block's rate is 0 (nothing is drawn)"""
        out = []
        for blocks, n in ((self.Spatial_blocks, b * self.num_frame), (self.blocks, b)):
            for blk in blocks:
                r = blk.rate()
                out.append(tuple(_drop_mask(n, 1.0 - r, device) for _ in range(2)) if r > 0.0 else (None, None))
        return out

    def forward(self, x, drop_masks=None):
        """drop_masks: a training forward's masks as drop_path_masks returns them (default: drawn here)"""
        f, p = self.num_frame, self.num_joints
        if x.numel() % (f * p * 2):
            raise ValueError("PoseTransformer: input must view as (-1, %d, %d, 2), got %s" % (f, p, tuple(x.shape)))
        x = x.reshape(-1, f, p, 2)
        b = x.shape[0]
        masks = None
        if self.training:
            masks = drop_masks if drop_masks is not None else self.drop_path_masks(b, x.device)
        if not x.is_cuda or (not self.training and torch.is_grad_enabled()):
            return self._forward_torch(x, masks)
        if self._arithmetic() not in PRECISIONS:
            raise ValueError("PoseTransformer.precision must be one of %s (or 'f16x3', which runs as 'bf16x6'), got %r"
                             % (PRECISIONS, self.precision))
        rows = x.float().reshape(b * f * p, 2)
        y = self._forward_train(rows, b, masks) if self.training else self._forward_eval(rows, b)
        return y.view(b, 1, p, 3)

    # ------------------------------------------------------------------------------------------------ plain torch
    def _forward_torch(self, x, masks):
        b, f, p = x.shape[0], self.num_frame, self.num_joints
        none = [(None, None)] * (2 * len(self.blocks))
        masks = none if masks is None else masks
        h = self.Spatial_patch_to_embedding(x.to(self.Spatial_pos_embed.dtype).reshape(b * f, p, 2)) + self.Spatial_pos_embed
        for blk, m in zip(self.Spatial_blocks, masks):
            h = blk(h, m)
        n = self.Spatial_norm
        h = F.layer_norm(h, n.normalized_shape, n.weight, n.bias, n.eps).reshape(b, f, p * self.embed_dim_ratio) + self.Temporal_pos_embed
        for blk, m in zip(self.blocks, masks[len(self.Spatial_blocks):]):
            h = blk(h, m)
        n = self.Temporal_norm
        h = F.layer_norm(h, n.normalized_shape, n.weight, n.bias, n.eps)
        h = torch.matmul(self.weighted_mean.weight.view(1, f), h).view(b, 1, -1) + self.weighted_mean.bias
        return self.head(h).view(b, 1, p, -1)

    # ------------------------------------------------------------------------------------------------ training
    def _block_train(self, x, blk, S, N, prec, masks):
        """x: the fp32 residual stream (S N, C)"""
        bf = prec == "bf16"
        att, mlp = blk.attn, blk.mlp
        keep = 1.0 - blk.rate()

        def add(y, m):
            return x + (y.view(S, -1) * (m / keep).view(S, 1)).view_as(x)

        h = A.layer_norm(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, out_bf16=bf)
        qkv = A.linear(h, att.qkv.weight, att.train_bias(), None, A.ACT_NONE, 0.0, prec, out_f32=not bf)
        o = A.attention(qkv, S, N, att.num_heads, att.head_dim, att.scale)
        if masks[0] is None:
            x = A.linear(o, att.proj.weight, att.proj.bias, x, A.ACT_NONE, 0.0, prec, out_f32=True)
        else:
            x = add(A.linear(o, att.proj.weight, att.proj.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True), masks[0])
        h = A.layer_norm(x, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, out_bf16=bf)
        z = A.linear(h, mlp.fc1.weight, mlp.fc1.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)
        a = A.gelu(z, out_bf16=bf)
        if masks[1] is None:
            return A.linear(a, mlp.fc2.weight, mlp.fc2.bias, x, A.ACT_NONE, 0.0, prec, out_f32=True)
        return add(A.linear(a, mlp.fc2.weight, mlp.fc2.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True), masks[1])

    def _forward_train(self, rows, b, masks):
        prec = self._arithmetic()
        f, p, Cs, Ct = self.num_frame, self.num_joints, self.embed_dim_ratio, self.embed_dim
        pe = self.Spatial_patch_to_embedding
        h = A.linear(rows, pe.weight, pe.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)
        h = (h.view(b * f, p, Cs) + self.Spatial_pos_embed).view(b * f * p, Cs)
        for blk, m in zip(self.Spatial_blocks, masks):
            h = self._block_train(h, blk, b * f, p, prec, m)
        n = self.Spatial_norm
        h = A.layer_norm(h, n.weight, n.bias, n.eps)
        h = (h.view(b, f, Ct) + self.Temporal_pos_embed).view(b * f, Ct)
        for blk, m in zip(self.blocks, masks[len(self.Spatial_blocks):]):
            h = self._block_train(h, blk, b, f, prec, m)
        n = self.Temporal_norm
        h = A.layer_norm(h, n.weight, n.bias, n.eps)
        h = torch.matmul(self.weighted_mean.weight.view(1, f), h.view(b, f, Ct)).view(b, Ct) + self.weighted_mean.bias
        n, lin = self.head[0], self.head[1]
        h = A.layer_norm(h, n.weight, n.bias, n.eps, out_bf16=prec == "bf16")
        return A.linear(h, lin.weight, lin.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)

    # ------------------------------------------------------------------------------------------------ evaluation
    def _block_eval(self, x, blk, S, N, prec):
        bf = prec == "bf16"
        att, mlp = blk.attn, blk.mlp
        ln = lambda t, n: ops.layernorm_forward(t, n.weight.detach(), n.bias.detach(), n.eps, out_bf16=bf, want_stats=False)[0]
        qkv = A.linear(ln(x, blk.norm1), att.qkv.weight, att.qkv.bias, None, A.ACT_NONE, 0.0, prec, out_f32=not bf)
        o = ops.attn_forward(qkv, S, N, att.num_heads, att.head_dim, att.scale, want_lse=False)[0]
        x = A.linear(o, att.proj.weight, att.proj.bias, x, A.ACT_NONE, 0.0, prec, out_f32=True)
        z = A.linear(ln(x, blk.norm2), mlp.fc1.weight, mlp.fc1.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)
        return A.linear(ops.gelu_forward(z, out_bf16=bf), mlp.fc2.weight, mlp.fc2.bias, x, A.ACT_NONE, 0.0, prec, out_f32=True)

    def _forward_eval(self, rows, b):
        prec = self._arithmetic()
        f, p, Cs, Ct = self.num_frame, self.num_joints, self.embed_dim_ratio, self.embed_dim
        ln = lambda t, n, bf=False: ops.layernorm_forward(t, n.weight.detach(), n.bias.detach(), n.eps, out_bf16=bf, want_stats=False)[0]
        pe = self.Spatial_patch_to_embedding
        h = A.linear(rows, pe.weight, pe.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)
        h = (h.view(b * f, p, Cs) + self.Spatial_pos_embed).view(b * f * p, Cs)
        for blk in self.Spatial_blocks:
            h = self._block_eval(h, blk, b * f, p, prec)
        h = (ln(h, self.Spatial_norm).view(b, f, Ct) + self.Temporal_pos_embed).view(b * f, Ct)
        for blk in self.blocks:
            h = self._block_eval(h, blk, b, f, prec)
        h = ln(h, self.Temporal_norm)
        h = torch.matmul(self.weighted_mean.weight.view(1, f), h.view(b, f, Ct)).view(b, Ct) + self.weighted_mean.bias
        lin = self.head[1]
        return A.linear(ln(h, self.head[0], prec == "bf16"), lin.weight, lin.bias, None, A.ACT_NONE, 0.0, prec, out_f32=True)
