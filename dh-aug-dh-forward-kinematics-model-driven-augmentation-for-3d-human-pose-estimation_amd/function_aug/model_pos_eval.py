"""Drop-ins for the posenet evaluation of R/function_aug/model_pos_eval.py (evaluate :16-92, evaluate_posenet :96-118).

The posenet calls are the reference's (model.eval(), no_grad, view(num_poses, -1), (out + out_flip) / 2.0 with the flip of
dhaug_center_flip); the metrics are summed on the device (utils.loss.PoseMetricsAccumulator) and read ONCE per call, at
the end, instead of a .cpu() / numpy pass per batch.  Batches may be host tensors (uploaded non_blocking; the reference's
loaders pin memory) or device tensors.  There is no per-batch progress bar (it would need per-batch host values): one
summary line is printed.  The returned averages are the global means over poses and joints, which equal the reference's
pose-weighted batch means."""
import torch

from .. import ops
from ..utils.loss import PoseMetricsAccumulator


def _poses(t, C, name):
    if t.dim() < 2 or t.numel() != t.shape[0] * 16 * C:
        raise ValueError("%s: expected %d joints x %d coordinates per pose, got %s" % (name, 16, C, tuple(t.shape)))
    return t.reshape(t.shape[0], 16, C)


def flip_pose(x):
    """x -> -x and the left / right joint swap of the reference's flip augmentation, for (..., 16, C) poses, C in {2, 3}"""
    return ops.center_flip(x, center=False, flip=True).reshape(x.shape)


def write_scalars(writer, summary, key, tag, flipaug, p1, p2, pck, auc):
    if writer:
        base = "posenet_{}".format(key) + flipaug
        writer.add_scalar(base + "/p1score" + tag, p1, summary.epoch)
        writer.add_scalar(base + "/p2score" + tag, p2, summary.epoch)
        writer.add_scalar(base + "/_pck" + tag, pck, summary.epoch)
        writer.add_scalar(base + "/_auc" + tag, auc, summary.epoch)


def finish(acc, get_pck_auc, key):
    """(p1 mm, p2 mm, pck %, auc %) from the accumulator's one host read"""
    r = acc.result()
    p1, p2 = r["mpjpe"] * 1000.0, r["p_mpjpe"] * 1000.0
    pck, auc = (r["pck"], r["auc"]) if get_pck_auc and r["poses"] else (0, 0)
    print("Eval posenet on {}: {} poses | MPJPE: {: .4f} | P-MPJPE: {: .4f} | PCK: {: .4f} | AUC: {: .4f}"
          .format(key, r["poses"], p1, p2, pck, auc))
    return p1, p2, pck, auc


def evaluate(data_loader, model_pos_eval, device, summary=None, writer=None,
             key='', tag='', flipaug='', get_pck_auc=False):
    model_pos_eval.eval()
    acc = PoseMetricsAccumulator(device, center=True)
    for temp in data_loader:
        targets_3d, inputs_2d = temp[0], temp[1]
        num_poses = targets_3d.size(0)
        targets_3d = _poses(targets_3d, 3, "targets_3d").to(device, non_blocking=True)
        inputs_2d = _poses(inputs_2d, 2, "inputs_2d").to(device, non_blocking=True)
        with torch.no_grad():
            if flipaug:
                inputs_2d_flip = flip_pose(inputs_2d)
                outputs_3d_flip = flip_pose(model_pos_eval(inputs_2d_flip.view(num_poses, -1)).view(num_poses, -1, 3))
                outputs_3d = model_pos_eval(inputs_2d.view(num_poses, -1)).view(num_poses, -1, 3)
                outputs_3d = (outputs_3d + outputs_3d_flip) / 2.0
            else:
                outputs_3d = model_pos_eval(inputs_2d.view(num_poses, -1)).view(num_poses, -1, 3)
        acc.add(outputs_3d, targets_3d)
    p1, p2, pck, auc = finish(acc, get_pck_auc, key)
    write_scalars(writer, summary, key, tag, flipaug, p1, p2, pck, auc)
    return p1, p2, pck, auc


def evaluate_posenet(args, data_dict, model_pos, model_pos_eval, device, summary, writer, tag, get_pck_auc=False):
    """H36M without and 3DHP with the test-time flip, as the reference"""
    with torch.no_grad():
        model_pos_eval.load_state_dict(model_pos.state_dict())
        h36m_p1, h36m_p2, _, _ = evaluate(data_dict['H36M_test'], model_pos_eval, device, summary, writer,
                                          key='H36M_test', tag=tag, flipaug='')
        dhp_p1, dhp_p2, PCK, AUC = evaluate(data_dict['mpi3d_loader'], model_pos_eval, device, summary, writer,
                                            key='mpi3d_loader', tag=tag, flipaug='_flip', get_pck_auc=get_pck_auc)
    return h36m_p1, h36m_p2, dhp_p1, dhp_p2, PCK, AUC
