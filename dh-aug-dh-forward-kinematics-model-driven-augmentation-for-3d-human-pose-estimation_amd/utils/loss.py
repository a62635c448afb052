"""Drop-ins for the evaluation metrics of R/utils/loss.py (mpjpe :8-14, p_mpjpe :123-164, compute_PCK / compute_AUC :192-225),
computed on the device by one dhaug_pose_metrics launch (plus its one-wave reduction).  mpjpe is also the criterion of the
reference's video command: called on a device tensor that requires grad it is differentiable (dhaug_pose_mpjpe).

Same signatures and return values as the reference for host (numpy / CPU tensor) inputs: they are uploaded, and one host
read returns what the reference returns (a CPU 0-d tensor for mpjpe, a numpy scalar for p_mpjpe, a float for compute_PCK,
a numpy float64 for compute_AUC).  Device tensors in: 0-d device tensors out, with no synchronisation.  Poses are
(..., 16, 3); anything else raises ValueError before a launch.

PoseMetricsAccumulator sums the same metrics over many batches in a device record and reads it once (evaluate in
function_aug/model_pos_eval.py and video_mode_evaluate use it)."""
import numpy as np
import torch

from .. import _lib, ops

AUC_THRESHOLDS = np.linspace(0, 150, 31)     # mm, compute_AUC's thresholds; the last one is compute_PCK's default 150
PCK_INDEX = 30


def _multiplicity(eval_joints):
    """eval_joints (np.take indices into the 16 joints, repeats allowed) -> per-joint counts and the number of columns"""
    if eval_joints is None:
        return None, 16
    idx = np.asarray(eval_joints).reshape(-1)
    if idx.size == 0 or not np.issubdtype(idx.dtype, np.integer) or idx.min() < -16 or idx.max() >= 16:
        raise ValueError("eval_joints must be indices into the 16 joints, got %r" % (eval_joints,))
    m = np.bincount(idx % 16, minlength=16)
    if m.max() > _lib.EVAL_MAX_MULTIPLICITY:
        raise ValueError("eval_joints repeats a joint more than %d times" % _lib.EVAL_MAX_MULTIPLICITY)
    return [int(v) for v in m], int(idx.size)


def _device_pair(pred, target, name):
    """(pred, target) as device fp32 (N, 16, 3) tensors; second value: True if the inputs were on the host"""
    sp, st = tuple(pred.shape), tuple(target.shape)
    if sp != st:
        raise ValueError("%s: predicted %s and target %s differ in shape" % (name, sp, st))
    if len(sp) < 2 or sp[-2:] != (16, 3):
        raise ValueError("%s: poses must be (..., 16, 3), got %s" % (name, sp))
    if torch.is_tensor(pred) and pred.is_cuda:
        return pred.reshape(-1, 16, 3), target.reshape(-1, 16, 3).to(pred.device), False
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a,
                                                         dtype=np.float32)).pin_memory().to("cuda", non_blocking=True)
    return up(pred).reshape(-1, 16, 3), up(target).reshape(-1, 16, 3), True


def _totals(pred, target, center=False, thresholds=(), multiplicity=None):
    tot = ops.eval_totals(pred.device)
    ops.pose_metrics(pred, target, center=center, thresholds=thresholds, multiplicity=multiplicity, totals=tot)
    return tot


def _f64(tot):
    return tot[:2].view(torch.float64)


class _MpjpeFn(torch.autograd.Function):
    """mpjpe as a training criterion: ops.pose_mpjpe gives the loss and d loss / d predicted in one launch pair; the gradient is
    kept for the backward.  First order only."""

    @staticmethod
    def forward(ctx, predicted, target):
        loss, grad = ops.pose_mpjpe(predicted, target, predicted.numel() // 48)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        g = grad_output * grad
        return g, (-g if ctx.needs_input_grad[1] else None)


def mpjpe(predicted, target):
    """mean per-joint position error (Protocol #1).  As a metric (no gradient asked for, or host inputs): the mean of the fp32
    joint distances from dhaug_pose_metrics.  As a criterion -- an fp32 device tensor that requires grad, with gradients enabled
    -- a 0-d tensor with a grad_fn over dhaug_pose_mpjpe (fp64 distances; a joint at distance 0 gets a zero gradient)."""
    y, x, host = _device_pair(predicted, target, "mpjpe")
    if not host and predicted.dtype == torch.float32 and predicted.requires_grad and torch.is_grad_enabled():
        return _MpjpeFn.apply(y, x.to(torch.float32))
    tot = _totals(y, x)
    v = _f64(tot)[0] / (16.0 * tot[2].double())
    dtype = predicted.dtype if torch.is_tensor(predicted) else torch.float32
    v = v.to(dtype if dtype.is_floating_point else torch.float32)
    return v.cpu() if host else v


def p_mpjpe(predicted, target):
    """mean per-joint position error after the optimal similarity alignment (Protocol #2), per pose in fp64"""
    y, x, host = _device_pair(predicted, target, "p_mpjpe")
    tot = _totals(y, x)
    v = _f64(tot)[1] / tot[2].double()
    if not host:
        return v.to(predicted.dtype if predicted.dtype.is_floating_point else torch.float32)
    both32 = all(getattr(a, "dtype", None) in (np.float32, torch.float32) for a in (predicted, target))
    return (np.float32 if both32 else np.float64)(v.item())


def compute_PCK(gts, preds, scales=1000, eval_joints=None, threshold=150):
    """percentage of joints (eval_joints columns) whose error in mm, fl32(e * 1000), is below threshold"""
    mult, cols = _multiplicity(eval_joints)
    y, x, host = _device_pair(preds, gts, "compute_PCK")
    tot = _totals(y, x, thresholds=[threshold], multiplicity=mult)
    if host:
        t = tot.cpu()
        return float(int(t[3]) / (int(t[2]) * cols)) * 100
    return tot[3].double() * 100.0 / (tot[2].double() * cols)


def compute_AUC(gts, preds, scales=1000, eval_joints=None):
    """mean of compute_PCK over the 31 thresholds 0, 5, ..., 150 mm"""
    mult, cols = _multiplicity(eval_joints)
    y, x, host = _device_pair(preds, gts, "compute_AUC")
    tot = _totals(y, x, thresholds=AUC_THRESHOLDS, multiplicity=mult)
    if host:
        t = tot.cpu().tolist()
        total = t[2] * cols
        return np.mean([float(t[3 + k] / total) * 100 for k in range(len(AUC_THRESHOLDS))])
    return (tot[3:3 + len(AUC_THRESHOLDS)].double() * 100.0 / (tot[2].double() * cols)).mean()


class PoseMetricsAccumulator:
    """MPJPE, P-MPJPE, PCK (150 mm) and AUC summed over batches in one device record; result() reads it once.

    center=True root-centres both poses first (what evaluate does).  add() enqueues one launch pair on the current stream
    and never synchronises."""

    def __init__(self, device=None, center=True, eval_joints=None):
        self.center = bool(center)
        self.mult, self.cols = _multiplicity(eval_joints)
        self.totals = ops.eval_totals(device)

    def zero(self):
        self.totals.zero_()
        return self

    def add(self, pred, target):
        y, x, _ = _device_pair(pred, target, "PoseMetricsAccumulator.add")
        ops.pose_metrics(y, x, center=self.center, thresholds=AUC_THRESHOLDS, multiplicity=self.mult, totals=self.totals)

    def result(self):
        """dict(poses, mpjpe, p_mpjpe in meters; pck, auc in %) from one host read; zeros for no poses"""
        t = self.totals.cpu().numpy()
        n = int(t[2])
        if n == 0:
            return dict(poses=0, mpjpe=0.0, p_mpjpe=0.0, pck=0.0, auc=0.0)
        se, sp = (float(v) for v in t[:2].view(np.float64))
        tp = [int(v) for v in t[3:3 + len(AUC_THRESHOLDS)]]
        total = n * self.cols
        return dict(poses=n, mpjpe=se / (16.0 * n), p_mpjpe=sp / n, pck=float(tp[PCK_INDEX] / total) * 100,
                    auc=float(np.mean([float(v / total) * 100 for v in tp])))
