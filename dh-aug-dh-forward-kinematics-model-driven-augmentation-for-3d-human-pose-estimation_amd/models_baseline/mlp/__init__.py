"""Drop-in for R/models_baseline/mlp: the "simple yet effective baseline" MLP posenet (`--posenet_name mlp`)."""
from .linear_model import Linear, LinearModel, init_weights

__all__ = ["Linear", "LinearModel", "init_weights"]
