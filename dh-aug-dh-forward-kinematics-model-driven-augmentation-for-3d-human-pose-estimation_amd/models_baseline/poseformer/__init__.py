"""PoseFormer posenet (`--posenet_name mulit_farme_poseformer`): drop-in for R/models_baseline/poseformer."""
from .model_poseformer import Attention, Block, DropPath, Mlp, PoseTransformer  # noqa: F401

__all__ = ["Attention", "Block", "DropPath", "Mlp", "PoseTransformer"]
