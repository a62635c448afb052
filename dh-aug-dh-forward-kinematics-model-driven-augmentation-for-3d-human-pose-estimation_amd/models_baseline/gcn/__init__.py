"""SemGCN posenet (`--posenet_name gcn`): drop-in for R/models_baseline/gcn."""
from .graph_utils import H36M_PARENTS, adj_mx_from_parents, adj_mx_from_skeleton  # noqa: F401
from .sem_gcn import SemGCN  # noqa: F401
from .sem_graph_conv import SemGraphConv  # noqa: F401
