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


# ------------------------------------------------------------------------------------------------------------------------
# The VideoPose3D family of R/utils/loss.py: mpjpe_byjoint :17-23, weighted_mpjpe :26-32, n_mpjpe :167-177 and
# mean_velocity_error :180-189, on dhaug_pose_column_errors / dhaug_pose_scaled_errors.  The module's conventions hold: poses
# are (..., 16, 3), host inputs are uploaded as fp32 and one host read returns the reference's type, device tensors in give
# device tensors out with no synchronisation.  Every distance, scale and sum is fp64 from the fp32 values; the result is
# rounded once to the returned type.  The three torch functions are criteria too: an fp32 device `predicted` that requires
# grad (gradients enabled, no gradient asked for target or w) goes through an autograd.Function over dhaug_pose_nmpjpe,
# dhaug_pose_wmpjpe or dhaug_pose_byjoint_backward (first order only); any other `predicted` that requires grad evaluates
# the reference's expression in plain torch, so training code that uses them as a loss keeps working.


def _check_pair(pred, target, name):
    """the shape checks of _device_pair alone; returns the shape"""
    sp, st = tuple(pred.shape), tuple(target.shape)
    if sp != st:
        raise ValueError("%s: predicted %s and target %s differ in shape" % (name, sp, st))
    if len(sp) < 2 or sp[-2:] != (16, 3):
        raise ValueError("%s: poses must be (..., 16, 3), got %s" % (name, sp))
    return sp


def _shaped_pair(pred, target, name):
    """_device_pair with the callers' shape kept: (pred, target, host)"""
    y, x, host = _device_pair(pred, target, name)
    shape = tuple(pred.shape)
    return y.reshape(shape), x.reshape(shape), host


def _joints(shape):
    """the number of joints of a (..., 16, 3) shape"""
    return int(np.prod(shape[:-1], dtype=np.int64))


def _check_columns(shape, name):
    """dhaug_pose_column_errors takes the axes between the first and the last as its columns"""
    if _joints(shape[1:]) > _lib.COLERR_MAX_COLS:
        raise ValueError("%s: %d joints per entry of the first axis, at most %d" % (name, _joints(shape[1:]), _lib.COLERR_MAX_COLS))


def _wants_grad(predicted):
    return torch.is_tensor(predicted) and predicted.requires_grad and torch.is_grad_enabled()


def takes_criterion_kernel(predicted, others=(), within_limits=True):
    """the rule that sends a call to the fused loss + gradient kernels, from attributes alone: `predicted` is an fp32 device
    tensor that requires grad, gradients are enabled, no other operand (target, w) requires grad, and the metric kernel's shape
    limits hold.  Anything else keeps the metric kernel or the plain-torch expression."""
    return bool(getattr(predicted, "is_cuda", False) and getattr(predicted, "dtype", None) == torch.float32
                and getattr(predicted, "requires_grad", False) and torch.is_grad_enabled()
                and not any(getattr(o, "requires_grad", False) for o in others) and within_limits)


def _f32_on(t, device):
    return t.detach().to(device=device, dtype=torch.float32)


class _ScalarCriterionFn(torch.autograd.Function):
    """n_mpjpe / weighted_mpjpe as training criteria, as _MpjpeFn is for mpjpe: ops.pose_nmpjpe (w None) or ops.pose_wmpjpe
    gives the loss and d loss / d predicted in one launch pair; the gradient is kept for the backward.  First order only."""

    @staticmethod
    def forward(ctx, predicted, target, w):
        poses = predicted.numel() // 48
        if w is None:
            loss, grad = ops.pose_nmpjpe(predicted, target, poses)
        else:
            loss, grad = ops.pose_wmpjpe(predicted, target, w, poses)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad_output * grad, None, None


class _ByJointFn(torch.autograd.Function):
    """mpjpe_byjoint as a training criterion: the value is the metric's (dhaug_pose_column_errors, the same bits), the backward
    one dhaug_pose_byjoint_backward launch over the saved operands.  First order only."""

    @staticmethod
    def forward(ctx, predicted, target):
        sp = tuple(predicted.shape)
        cols = torch.zeros(_joints(sp[1:]), dtype=torch.float64, device=predicted.device)
        ops.pose_column_errors(predicted, target, col_sums=cols)
        ctx.save_for_backward(predicted, target)
        return (cols / float(sp[0])).reshape(sp[1:-1]).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        predicted, target = ctx.saved_tensors
        return ops.pose_byjoint_backward(predicted, target, grad_output), None


def _result(v, predicted, host):
    """v (fp64 device tensor) as the torch functions return it: predicted's floating dtype, on the host for host inputs"""
    dtype = predicted.dtype if torch.is_tensor(predicted) else torch.float32
    v = v.to(dtype if dtype.is_floating_point else torch.float32)
    return v.cpu() if host else v


def mpjpe_byjoint(predicted, target):
    """the joint error averaged over the FIRST axis only: (N, 16, 3) gives (16,), (B, F, 16, 3) gives (F, 16) -- the shape is
    predicted.shape[1:-1].  fp64 distances and sums (dhaug_pose_column_errors).  As a criterion (takes_criterion_kernel) the same
    value with a grad_fn over dhaug_pose_byjoint_backward; any other `predicted` that requires grad -- and the one-pose form,
    and more than COLERR_MAX_COLS joints per entry -- is evaluated in plain torch (differentiable), not on the kernel."""
    sp = _check_pair(predicted, target, "mpjpe_byjoint")
    if takes_criterion_kernel(predicted, (target,), len(sp) > 2 and _joints(sp[1:]) <= _lib.COLERR_MAX_COLS):
        return _ByJointFn.apply(predicted, _f32_on(target, predicted.device))
    if _wants_grad(predicted):
        return torch.mean(torch.norm(predicted - target.to(predicted.device), dim=-1), dim=0)
    if len(sp) == 2:                                  # one pose: the first axis is the joints
        return mpjpe(predicted, target)
    _check_columns(sp, "mpjpe_byjoint")
    y, x, host = _shaped_pair(predicted, target, "mpjpe_byjoint")
    cols = torch.zeros(_joints(sp[1:]), dtype=torch.float64, device=y.device)
    ops.pose_column_errors(y, x, col_sums=cols)
    return _result((cols / float(sp[0])).reshape(sp[1:-1]), predicted, host)


def _weights(w, shape, name):
    """w against the joint-error shape (predicted.shape[:-1]) under torch broadcasting, checked; w stays as given in
    the per-pose (..., 1) and per-joint forms, any other broadcastable form is expanded to one value per joint"""
    ws = tuple(w.shape)
    if len(ws) == 0 or ws[0] != shape[0]:
        raise ValueError("%s: w %s must have predicted's first dimension (%d)" % (name, ws, shape[0]))
    try:
        out = tuple(torch.broadcast_shapes(ws, shape))
    except RuntimeError:
        raise ValueError("%s: w %s does not broadcast against the joint errors %s" % (name, ws, shape)) from None
    if out != shape:
        raise ValueError("%s: w %s would enlarge the joint errors %s to %s" % (name, ws, shape, out))
    if ws == shape or ws == shape[:-1] + (1,):
        return w
    return w.expand(shape)


def weighted_mpjpe(predicted, target, w):
    """mean(w * norm(predicted - target, dim=-1)) under torch broadcasting of w against predicted.shape[:-1]: one weight per
    joint, per pose ((..., 1)), or any shape that broadcasts to these without enlarging the result; w.shape[0] must be
    predicted.shape[0].  Weights of any sign.  fp64 distances and sums (dhaug_pose_scaled_errors).  As a criterion
    (takes_criterion_kernel) a 0-d tensor with a grad_fn over dhaug_pose_wmpjpe; any other `predicted` that requires grad is
    evaluated in plain torch (differentiable), not on the kernel."""
    sp = _check_pair(predicted, target, "weighted_mpjpe")
    w = _weights(w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w)), sp[:-1], "weighted_mpjpe")
    if takes_criterion_kernel(predicted, (target, w)):
        return _ScalarCriterionFn.apply(predicted, _f32_on(target, predicted.device), _f32_on(w, predicted.device))
    if _wants_grad(predicted):
        return torch.mean(w.to(predicted.device) * torch.norm(predicted - target.to(predicted.device), dim=-1))
    y, x, host = _shaped_pair(predicted, target, "weighted_mpjpe")
    sums = ops.pose_scaled_errors(y, x, w=w.detach().to(device=y.device, dtype=torch.float32))
    return _result(sums[1] / float(_joints(sp)), predicted, host)


def n_mpjpe(predicted, target):
    """scale-normalised MPJPE of (B, F, 16, 3) poses: per frame s = mean_j(sum target * predicted) / mean_j(sum predicted^2),
    then mpjpe(s * predicted, target).  fp64 scale, distances and sums (dhaug_pose_scaled_errors); an all-zero predicted frame
    gives NaN, as the reference.  As a criterion (takes_criterion_kernel) a 0-d tensor with a grad_fn over dhaug_pose_nmpjpe
    (a frame the prediction fits exactly up to scale gets a zero gradient); any other `predicted` that requires grad is
    evaluated in plain torch (differentiable), not on the kernel."""
    if len(tuple(predicted.shape)) != 4:
        raise ValueError("n_mpjpe: poses must be (B, F, 16, 3), got %s" % (tuple(predicted.shape),))
    sp = _check_pair(predicted, target, "n_mpjpe")
    if takes_criterion_kernel(predicted, (target,)):
        return _ScalarCriterionFn.apply(predicted, _f32_on(target, predicted.device), None)
    if _wants_grad(predicted):
        target = target.to(predicted.device)
        norm_predicted = torch.mean(torch.sum(predicted ** 2, dim=3, keepdim=True), dim=2, keepdim=True)
        norm_target = torch.mean(torch.sum(target * predicted, dim=3, keepdim=True), dim=2, keepdim=True)
        return torch.mean(torch.norm(norm_target / norm_predicted * predicted - target, dim=-1))
    y, x, host = _shaped_pair(predicted, target, "n_mpjpe")
    sums = ops.pose_scaled_errors(y, x)
    return _result(sums[0] / float(_joints(sp)), predicted, host)


class JointWeightedMpjpe:
    """weighted_mpjpe with sixteen per-joint weights shared by every pose, as a criterion object: callable (predicted, target).
    The weights are kept as one fp32 buffer, moved to the device on first use and read there in place by dhaug_pose_wmpjpe
    (DHAUG_WMPJPE_SHARED) -- StepRunner fuses an instance of this class, and a captured step holds the buffer's address.  A call
    that takes_criterion_kernel does not send to the kernels (host inputs, fp64, no gradient asked for, ...) is
    weighted_mpjpe(predicted, target, weights.expand(predicted.shape[:-1])): the same value, evaluated as that function does."""

    def __init__(self, weights):
        w = torch.as_tensor(weights).detach().to(torch.float32).reshape(-1)
        if w.numel() != 16:
            raise ValueError("JointWeightedMpjpe: sixteen weights, one per joint, got %d" % w.numel())
        self.weights = w.clone().contiguous()

    def buffer(self, device):
        """the sixteen weights as an fp32 tensor on `device` (moved once; the same tensor from then on)"""
        d, have = torch.device(device), self.weights.device
        if have.type != d.type or (d.index is not None and have.index != d.index):
            self.weights = self.weights.to(d).contiguous()
        return self.weights

    def __call__(self, predicted, target):
        sp = _check_pair(predicted, target, "JointWeightedMpjpe")
        if takes_criterion_kernel(predicted, (target,)):
            return _ScalarCriterionFn.apply(predicted, _f32_on(target, predicted.device), self.buffer(predicted.device))
        w = self.buffer(predicted.device) if torch.is_tensor(predicted) and predicted.is_cuda else self.weights
        return weighted_mpjpe(predicted, target, w.expand(sp[:-1]))

    def __repr__(self):
        return "JointWeightedMpjpe(%s)" % (self.weights.tolist(),)


def mean_velocity_error(predicted, target):
    """mean per-joint velocity error of a sequence (frames, ..., 16, 3): mean(norm(diff(predicted, axis=0) - diff(target,
    axis=0), axis=-1)), fp64 differences, distances and sums (dhaug_pose_column_errors).  Host inputs (numpy or CPU tensors):
    a numpy scalar, float32 when both inputs are fp32, else float64.  Device tensors: a 0-d device tensor.  Fewer than two
    frames give NaN without a launch."""
    sp = _check_pair(predicted, target, "mean_velocity_error")
    if len(sp) < 3:
        raise ValueError("mean_velocity_error: a sequence must be (frames, ..., 16, 3), got %s" % (sp,))
    _check_columns(sp, "mean_velocity_error")
    host = not (torch.is_tensor(predicted) and predicted.is_cuda)
    both32 = all(getattr(a, "dtype", None) in (np.float32, torch.float32) for a in (predicted, target))
    if sp[0] < 2:
        if host:
            return (np.float32 if both32 else np.float64)(np.nan)
        return torch.full((), float("nan"), dtype=predicted.dtype if predicted.dtype.is_floating_point else torch.float32,
                          device=predicted.device)
    y, x, host = _shaped_pair(predicted, target, "mean_velocity_error")
    vel = ops.pose_column_errors(y, x, vel_sum=torch.zeros(1, dtype=torch.float64, device=y.device))[1]
    v = vel[0] / float((sp[0] - 1) * _joints(sp[1:]))
    if not host:
        return v.to(predicted.dtype if predicted.dtype.is_floating_point else torch.float32)
    return (np.float32 if both32 else np.float64)(v.item())


class PoseDetailAccumulator:
    """per-joint MPJPE, N-MPJPE and the velocity error summed over batches in one device record; result() reads it once.

    center=True root-centres both poses first (what evaluate does).  add() enqueues its launches on the current stream and
    never synchronises; the counts (poses, velocity pairs) follow from the shapes and are kept on the host."""

    def __init__(self, device=None, center=True):
        self.center = bool(center)
        self.record = torch.zeros(19, dtype=torch.float64, device=device if device is not None else "cuda")
        self.poses = 0
        self.velocity_pairs = 0

    def zero(self):
        self.record.zero_()
        self.poses = self.velocity_pairs = 0
        return self

    def add(self, pred, target, sequence=False):
        """(..., 16, 3) poses.  sequence=True: the first axis is the frames of ONE sequence, whose velocity error is accumulated
        too (one call per sequence: no pair is formed across calls)."""
        y, x, _ = _shaped_pair(pred, target, "PoseDetailAccumulator.add")
        col, nm, vel = self.record[:16], self.record[16:18], self.record[18:]
        y3, x3 = y.reshape(-1, 16, 3), x.reshape(-1, 16, 3)
        pairs = 0
        if sequence:
            if y.dim() < 3:
                raise ValueError("PoseDetailAccumulator.add: a sequence must be (frames, ..., 16, 3), got %s" % (tuple(y.shape),))
            pairs = max(0, y.shape[0] - 1) * (y[0].numel() // 3)
        if y3.shape[0] == 0:
            return
        if sequence and y.dim() == 3:
            ops.pose_column_errors(y3, x3, center=self.center, col_sums=col, vel_sum=vel)
        else:
            ops.pose_column_errors(y3, x3, center=self.center, col_sums=col)
            if pairs:
                ops.pose_column_errors(y, x, center=self.center, vel_sum=vel)
        ops.pose_scaled_errors(y3, x3, center=self.center, sums=nm)
        self.poses += y3.shape[0]
        self.velocity_pairs += pairs

    def result(self):
        """dict(poses, mpjpe_byjoint (16 floats), n_mpjpe, velocity in meters, velocity_pairs) from one host read; zeros where
        nothing was added"""
        t = self.record.cpu().numpy()
        n, pairs = self.poses, self.velocity_pairs
        return dict(poses=n, mpjpe_byjoint=[float(v) / n if n else 0.0 for v in t[:16]],
                    n_mpjpe=float(t[16]) / (16.0 * n) if n else 0.0,
                    velocity=float(t[18]) / pairs if pairs else 0.0, velocity_pairs=pairs)


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
