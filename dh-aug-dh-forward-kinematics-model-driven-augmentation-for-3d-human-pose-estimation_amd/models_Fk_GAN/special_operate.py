"""Hot-path symbols of R/models_Fk_GAN/special_operate.py: myResNet (:490-510), Fk_get_boneVecByPose3d (:513-539), and its three
DOF-distribution drawing functions (:347-485) over the device-side histograms of utils/dof_stats.py."""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import autograd_ops as A
from ..utils.dof_stats import DofDistribution

# (parent, child) joints of the 15 bones, FK bone order (R/models_Fk_GAN/forward_kinematics_DH_model.py:46-49)
BONE_PARENT = [5, 2, 4, 1, 0, 0, 0, 7, 8, 8, 10, 13, 11, 14, 8]
BONE_CHILD = [6, 3, 5, 2, 4, 1, 7, 8, 10, 13, 11, 14, 12, 15, 9]


class myResNet(nn.Module):
    """relu(fc2(relu(fc1(x))) + x); state_dict keys fc1.{weight,bias}, fc2.{weight,bias} as in the reference.
    Both layers run as bf16 MFMA GEMMs with bias / ReLU / residual fused into the epilogue."""

    def __init__(self, DIM):
        super().__init__()
        self.fc1 = nn.Linear(DIM, DIM)
        self.fc2 = nn.Linear(DIM, DIM)

    def forward(self, input, prec="bf16"):
        return A.res_block(input, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, A.ACT_RELU, 0.0, prec)


def Fk_get_boneVecByPose3d(x, num_joints=16):
    """(N,16,3) -> (N,15,3) child - parent.  The reference multiplies by a dense +-1 (16x15) matrix repeated N
    times; its two call sites (bone lengths, KCS) are fused HIP kernels here (dhaug_bone_length, dhaug_kcs_*), so
    this accessor is plain index arithmetic kept for API completeness."""
    p = torch.as_tensor(BONE_PARENT, device=x.device)
    c = torch.as_tensor(BONE_CHILD, device=x.device)
    return x[:, c] - x[:, p]


# ------------------------------------------------------------------ DOF angle distributions (R :347-485)
def _dof_table(angle_data):
    """(data_num, DOF_num) angles as an fp32 device table (the reference's .view(data_num, DOF_num))"""
    a = angle_data if torch.is_tensor(angle_data) else torch.as_tensor(np.ascontiguousarray(angle_data, dtype=np.float32))
    a = a.detach().reshape(a.shape[0], -1)
    if not a.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("the DOF distributions are computed on a GPU (no CPU fallback exists)")
        a = a.cuda()
    return a.float()


def _dof_figure(args, name, draw):
    """<checkpoint>/tmp/<name>.jpg through matplotlib when args.record_all_picture is true and matplotlib imports; nothing
    otherwise (the reference needs cv2 for the pair figures: not used here)"""
    if not getattr(args, "record_all_picture", False):
        return
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return
    folder = os.path.join(args.checkpoint, "tmp")
    os.makedirs(folder, exist_ok=True)
    fig = plt.figure()
    try:
        draw(fig.add_subplot(111), plt)
        fig.savefig(os.path.join(folder, name + ".jpg"))
    finally:
        plt.close(fig)


def my_draw_DOF_angle_distribute(angle_data, name, args):
    """R :347-410: the (DOF_num, 361) table of one-degree bins (bin = int(angle) + 180), each row over its maximum -- built
    on the device instead of in two nested Python loops, and RETURNED (numpy float64; the reference returns None).  Drawn as
    the reference's 'DOF angle heatmap' when args.record_all_picture is true and matplotlib imports."""
    a = _dof_table(angle_data)
    table = DofDistribution(a.shape[1], device=a.device).add(a).normalised()

    def draw(ax, plt):
        band = 10                                    # image rows per slot
        ax.matshow(np.repeat(table, band, axis=0), cmap="Blues")
        ax.set(title="DOF angle heatmap", xlabel="angle", ylabel="DOF ID")
        degrees = list(range(-180, 181, 60))
        ax.set_xticks([v + 180 for v in degrees], labels=degrees)
        slots = list(range(0, table.shape[0], 5))
        ax.set_yticks([band * s for s in slots], labels=slots)
    _dof_figure(args, name, draw)
    return table


def _draw_pair(all_angle_data, name, args, pair):
    a = _dof_table(all_angle_data)
    table = DofDistribution(a.shape[1], pairs=(pair,), device=a.device).add(a).result()["pair_counts"][0]

    def draw(ax, plt):
        # (the reference flips the image: the first slot's angle grows upwards)
        ax.imshow(table[::-1] / max(1, int(table.max())), cmap="jet")
        ax.set_axis_off()
    _dof_figure(args, name, draw)
    return table


def my_draw_distribute_for_paper(all_angle_data, name, args):
    """R :420-451: the 361 x 361 joint table of slots 8 and 3 of the generator's angles, table[bin(a_8)][bin(a_3)], raw
    int64 counts, returned (the reference returns None); drawn under the same conditions as my_draw_DOF_angle_distribute."""
    return _draw_pair(all_angle_data, name, args, (8, 3))


def my_draw_original_dataset_distribute_for_paper(all_angle_data, name, args):
    """R :454-485: the same for slots 0 and 1 of a dataset's angles."""
    return _draw_pair(all_angle_data, name, args, (0, 1))
