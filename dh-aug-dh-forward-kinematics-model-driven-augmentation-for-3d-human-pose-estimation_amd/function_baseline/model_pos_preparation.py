"""Drop-in for R/function_baseline/model_pos_preparation.py (model_pos_preparation :18-87): builds the posenet the augmentation
trains.  This package implements the reference's five posenet names, each through a factory of its own: `videopose` (the
default run's single-frame model, model_pos_preparation), `mulit_farme_videopose` (multi_frame_model_pos_preparation), `gcn`
(gcn_model_pos_preparation), `mlp` (mlp_model_pos_preparation) and `mulit_farme_poseformer` (poseformer_model_pos_preparation)."""
import torch

from ..models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f

POSENETS = ("videopose",)
REFERENCE_POSENETS = ("gcn", "mlp", "videopose", "mulit_farme_videopose", "mulit_farme_poseformer")


def _finish(args, name, model_pos, device, described):
    """the factories' common tail: the line that describes the model (`described` with the parameter count and the precision put
    behind it), then, with args.pretrain, ckpt['model_pos'] of args.posenet_pretrain_path; otherwise the constructors'
    initialisation stays (the reference applies its init_weights here, which touches nn.Linear modules only: of these models only
    the MLP holds any, and its factory has applied it by then)"""
    count = sum(p.numel() for p in model_pos.parameters())
    print("posenet %s, %d parameters (%.2f M), precision %s" % (described, count, count / 1e6, model_pos.precision))
    if getattr(args, "pretrain", False):
        path = getattr(args, "posenet_pretrain_path", None)
        if not path:
            raise ValueError("args.pretrain is set: give the checkpoint as args.posenet_pretrain_path")
        model_pos.load_state_dict(torch.load(path, map_location=device)['model_pos'])
        print("posenet %s: weights loaded from %s" % (name, path))
    return model_pos


def model_pos_preparation(args, dataset, device, flag='train'):
    """posenet (B,16,2) -> (B,16,3) for args.posenet_name, on `device`.  args.pretrain: load ckpt['model_pos'] from
    args.posenet_pretrain_path (the reference globs a hard-coded empty pattern there, so the path is an attribute of its own)."""
    name = args.posenet_name
    if name != 'videopose':
        known = "a posenet of the reference" if name in REFERENCE_POSENETS else "no posenet name at all"
        raise NotImplementedError("posenet_name %r (%s) is not implemented; implemented: %s" % (name, known, ", ".join(POSENETS)))
    widths = [1] * (int(args.stages) + 1)
    model_pos = TemporalModelOptimized1f(16, 2, 15, filter_widths=widths, causal=False, dropout=0.25, channels=1024).to(device)
    return _finish(args, name, model_pos, device, "%s: %d stages" % (name, len(widths) - 1))


MULTI_FRAME_POSENETS = ("mulit_farme_videopose",)


def multi_frame_model_pos_preparation(args, dataset, device, flag='train'):
    """the reference's `mulit_farme_videopose` branch (R/function_baseline/model_pos_preparation.py:42-50): posenet
    (B, T, 16, 2) -> (B, T', 16, 3) with filter widths args.architecture ('3,3', '3,3,3', ...); flag 'train' builds the strided
    multiFrame_TemporalModelOptimized1f, 'test' the dilated multiFrame_TemporalModel.  A factory of its own: model_pos_preparation
    above keeps refusing every name but `videopose`."""
    from ..models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModel, multiFrame_TemporalModelOptimized1f
    name = args.posenet_name
    if name not in MULTI_FRAME_POSENETS:
        raise NotImplementedError("posenet_name %r is not a multi-frame posenet of this package; implemented: %s"
                                  % (name, ", ".join(MULTI_FRAME_POSENETS)))
    if flag not in ("train", "test"):
        raise ValueError("flag must be 'train' or 'test', got %r" % (flag,))
    widths = [int(w) for w in str(args.architecture).split(',')]
    cls = multiFrame_TemporalModelOptimized1f if flag == "train" else multiFrame_TemporalModel
    model_pos = cls(16, 2, 16, filter_widths=widths, causal=False, dropout=0.25, channels=1024).to(device)
    return _finish(args, name, model_pos, device,
                   "%s (%s): filter widths %s, receptive field %d" % (name, cls.__name__, widths, model_pos.receptive_field()))


GCN_POSENETS = ("gcn",)


def gcn_model_pos_preparation(args, dataset, device, flag='train'):
    """the reference's `gcn` branch (R/function_baseline/model_pos_preparation.py:28-30): the SemGCN posenet (B, 16, 2) -> (B, 16, 3),
    SemGCN(adj, 128, num_layers=args.stages, p_dropout=args.dropout), the adjacency from dataset.skeleton() where the dataset has
    one and from the 16-joint Human3.6M parents otherwise.  A factory of its own: model_pos_preparation above keeps refusing
    every name but `videopose`."""
    from ..models_baseline.gcn import H36M_PARENTS, SemGCN, adj_mx_from_parents, adj_mx_from_skeleton
    name = args.posenet_name
    if name not in GCN_POSENETS:
        raise NotImplementedError("posenet_name %r is not a graph-convolution posenet of this package; implemented: %s"
                                  % (name, ", ".join(GCN_POSENETS)))
    skeleton = getattr(dataset, "skeleton", None)
    adj = adj_mx_from_skeleton(skeleton()) if callable(skeleton) else adj_mx_from_parents(H36M_PARENTS)
    model_pos = SemGCN(adj, 128, num_layers=int(args.stages), p_dropout=args.dropout, nodes_group=None).to(device)
    return _finish(args, name, model_pos, device, "%s: %d stages" % (name, int(args.stages)))


MLP_POSENETS = ("mlp",)


def mlp_model_pos_preparation(args, dataset, device, flag='train'):
    """the reference's `mlp` branch (R/function_baseline/model_pos_preparation.py:31-32): the MLP posenet (B, 16, 2) -> (B, 16, 3),
    LinearModel(32, 45, num_stage=args.stages, p_dropout=args.dropout).  Without args.pretrain the weights are init_weights'
    (kaiming_normal_), drawn on the HOST generator before the move to `device`: on a CPU device one seed gives the reference's
    weights; on a GPU device the reference draws them from the device generator (it moves the model first), so the same seed gives
    other weights there.  A factory of its own: model_pos_preparation above keeps refusing every name but `videopose`."""
    from ..models_baseline.mlp import LinearModel, init_weights
    name = args.posenet_name
    if name not in MLP_POSENETS:
        raise NotImplementedError("posenet_name %r is not an MLP posenet of this package; implemented: %s"
                                  % (name, ", ".join(MLP_POSENETS)))
    model_pos = LinearModel(32, 45, num_stage=int(args.stages), p_dropout=args.dropout)
    if not getattr(args, "pretrain", False):
        model_pos.apply(init_weights)
    model_pos = model_pos.to(device)
    return _finish(args, name, model_pos, device, "%s: %d stages" % (name, int(args.stages)))


POSEFORMER_POSENETS = ("mulit_farme_poseformer",)


def poseformer_model_pos_preparation(args, dataset, device, flag='train'):
    """the reference's `mulit_farme_poseformer` branch (R/function_baseline/model_pos_preparation.py:51-63): the PoseFormer posenet
    (B, T, J, 2) -> (B, 1, J, 3), PoseTransformer(num_frame = the receptive field of args.architecture, num_joints from
    dataset.skeleton() where the dataset has one and 16 otherwise, in_chans=2, embed_dim_ratio=32, depth=4, num_heads=8, mlp_ratio=2.,
    qkv_bias=True, qk_scale=None) with drop_path_rate 0.1 for flag 'train' and 0 for 'test'.  Without args.pretrain the nn.Linear
    weights are init_weights' (kaiming_normal_), drawn on the HOST generator before the move to `device`, as in
    mlp_model_pos_preparation.  A factory of its own: the four above keep refusing this name."""
    from ..models_baseline.mlp import init_weights
    from ..models_baseline.poseformer import PoseTransformer
    from ..models_Fk_GAN.video_mode_operate import video_receptive_field
    name = args.posenet_name
    if name not in POSEFORMER_POSENETS:
        raise NotImplementedError("posenet_name %r is not a transformer posenet of this package; implemented: %s"
                                  % (name, ", ".join(POSEFORMER_POSENETS)))
    if flag not in ("train", "test"):
        raise ValueError("flag must be 'train' or 'test', got %r" % (flag,))
    receptive_field = video_receptive_field([int(w) for w in str(args.architecture).split(',')])
    skeleton = getattr(dataset, "skeleton", None)
    num_joints = skeleton().num_joints() if callable(skeleton) else 16
    model_pos = PoseTransformer(num_frame=receptive_field, num_joints=num_joints, in_chans=2, embed_dim_ratio=32, depth=4, num_heads=8,
                                mlp_ratio=2., qkv_bias=True, qk_scale=None, drop_path_rate=0.1 if flag == "train" else 0)
    if not getattr(args, "pretrain", False):
        model_pos.apply(init_weights)
    model_pos = model_pos.to(device)
    return _finish(args, name, model_pos, device, "%s (%s): %d frames, %d joints" % (name, flag, receptive_field, num_joints))
