"""Drop-in for the posenet training loop of R/function_aug/model_pos_train.py (train_posenet :13-83), and the step machinery
the video loops of models_Fk_GAN/video_mode_operate.py share with it.

The posenet is whatever nn.Module the caller passes; what runs in this package's kernels is everything around its call:
  * the batch: one dhaug_pair_batch launch makes the root-centred targets, the inputs and their flipped / frame-reversed copies
    (for FakePairBuffer / TensorLoader sources from ONE permutation per epoch and index slices, for any other loader after the
    upload);
  * nn.MSELoss(reduction='mean'): dhaug_pose_mse gives the loss, its gradient (the loop calls outputs.backward(grad)) and the
    epoch's loss meter, AverageMeter.update(loss, num_poses) on the device;
  * utils.loss.mpjpe of this package (the criterion of the reference's video command): dhaug_pose_mpjpe, the same way;
  * nn.utils.clip_grad_norm_(max_norm=1) + optimizer.step(): optimizer.clip_step(1) of optim.PosenetAdam, two launches.
Each piece falls back on its own to what the reference calls (criterion(...).backward(), clip_grad_norm_, optimizer.step() of a
stock torch optimizer) when it does not apply; the loss still goes to the meter on the device.  Nothing is read on the host per
batch: the meters are read once when the loop ends and one summary line replaces the progress bar.  The loops return None as
the reference's do; the epoch's averages stay on <function>.last_meters, the per-step losses and gradient norms (device
tensors, never read here) on <function>.last_trace."""
import torch
import torch.nn as nn

from .. import ops
from ..optim import PosenetAdam
from ..utils.loss import mpjpe

METERS = ("loss", "flip_loss", "back_loss", "back_flip_loss")
_TRACE_CHUNK = 1024


def posenet_optimizer(model_pos, lr=1e-3):
    """the optimizer of the reference's posenet (torch.optim.Adam(model_pos.parameters(), lr)) on flat buffers, with clip_step"""
    return PosenetAdam(model_pos.parameters(), lr=lr)


def set_grad(nets, requires_grad=False):
    for net in nets:
        for p in net.parameters():
            p.requires_grad = requires_grad


class StepRunner:
    """One epoch's training steps.  step(inputs, targets, meter) = the reference's

        outputs = model_pos(inputs); optimizer.zero_grad(); loss = criterion(outputs, targets); loss.backward()
        nn.utils.clip_grad_norm_(model_pos.parameters(), max_norm=1); optimizer.step(); meter.update(loss.item(), num_poses)

    with the loss, the meter and the norm kept on the device."""

    def __init__(self, model_pos, optimizer, criterion, device):
        self.model, self.opt, self.criterion = model_pos, optimizer, criterion
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the posenet training loops need a GPU (no CPU fallback exists)")
        # the fused criteria: nn.MSELoss(reduction='mean') and this package's mpjpe; any other callable is called as it is
        self.fused_loss = None
        if isinstance(criterion, nn.MSELoss) and criterion.reduction == "mean":
            self.fused_loss = ops.pose_mse
        elif criterion is mpjpe:
            self.fused_loss = ops.pose_mpjpe
        self.fused_opt = hasattr(optimizer, "clip_step")
        self.meters = ops.loss_meters(len(METERS), self.device)
        self.workspace = ops.posetrain_workspace(self.device)
        self.trace = []                 # (chunk, 2) fp32 device tensors: loss and gradient norm of every step
        self.steps = 0

    def _slot(self):
        k = self.steps % _TRACE_CHUNK
        if k == 0:
            self.trace.append(torch.zeros((_TRACE_CHUNK, 2), dtype=torch.float32, device=self.device))
        self.steps += 1
        row = self.trace[-1][k]
        return row[0:1], row[1:2]

    def step(self, inputs, targets, meter, num_poses):
        loss_slot, norm_slot = self._slot()
        rec = None if meter is None else self.meters[METERS.index(meter)]
        outputs = self.model(inputs)
        self.opt.zero_grad()
        if self.fused_loss is not None:
            if tuple(outputs.shape) != tuple(targets.shape):
                raise ValueError("posenet output %s and target %s differ in shape" % (tuple(outputs.shape), tuple(targets.shape)))
            _, grad = self.fused_loss(outputs, targets, num_poses, meter=rec, workspace=self.workspace, loss=loss_slot)
            outputs.backward(grad.view(outputs.shape))
        else:
            loss = self.criterion(outputs, targets)
            loss.backward()
            with torch.no_grad():
                loss_slot.copy_(loss.detach().reshape(1))
                if rec is not None:
                    rec[0:1].view(torch.float64).add_(loss_slot.double(), alpha=num_poses)
                    rec[1:2] += num_poses
                    rec[2:3] += 1
        if self.fused_opt:
            self.opt.clip_step(1, norm_out=norm_slot)
        else:
            norm = nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=1)
            self.opt.step()
            norm_slot.copy_(norm.detach().reshape(1))

    def finish(self, flip):
        """the one host read: the meters' averages as a dict; the trace stays on the device"""
        if flip:
            # the reference updates its flip meter with the PLAIN step's loss (flip_epoch_loss_3d_pos.update(loss_3d_pos.item(),
            # num_poses): R/function_aug/model_pos_train.py:69, R/models_Fk_GAN/video_mode_operate.py:614,734), once per batch like
            # the plain meter: the two meters are equal, so the flip meter is the plain one's copy.  Reproduced on purpose.
            self.meters[METERS.index("flip_loss")].copy_(self.meters[METERS.index("loss")])
        raw = self.meters.cpu()
        sums = raw[:, 0:1].contiguous().view(torch.float64).reshape(-1).tolist()
        out = {}
        for k, name in enumerate(METERS):
            poses, steps = int(raw[k, 1]), int(raw[k, 2])
            out[name] = sums[k] / poses if poses else 0.0
            out[name + "_poses"], out[name + "_steps"] = poses, steps
        out["steps"] = self.steps
        return out

    def trace_tensor(self):
        if not self.trace:
            return torch.zeros((0, 2), dtype=torch.float32, device=self.device)
        return torch.cat(self.trace)[:self.steps]


def flat_source(data_loader):
    """(p3, p2) device tensors of a loader that keeps its pairs on the device (FakePairBuffer, TensorLoader), else None"""
    from ..models_Fk_GAN.model_fk_gan_train import FakePairBuffer
    from .dataloader_update import TensorLoader
    if isinstance(data_loader, FakePairBuffer):
        if not data_loader.p3:
            return None
        p3, p2, _ = data_loader.tensors()
    elif isinstance(data_loader, TensorLoader) and len(data_loader.tensors) >= 2:
        p3, p2 = data_loader.tensors[0], data_loader.tensors[1]
    else:
        return None
    if not (torch.is_tensor(p3) and torch.is_tensor(p2) and p3.is_cuda and p2.is_cuda):
        return None
    if tuple(p3.shape[-2:]) != (16, 3) or tuple(p2.shape[-2:]) != (16, 2) or p3.dim() not in (3, 4) or p2.dim() not in (3, 4):
        return None
    return p3, p2


def pair_batches(data_loader, device, flip, playback, pick):
    """the epoch's batches as dicts of dhaug_pair_batch.  Device-resident pair sources: one permutation per epoch (what their
    own iterator draws) and one launch per batch over an index slice; any other loader: pick(batch) -> (3D, 2D), uploaded."""
    from ..models_Fk_GAN.video_mode_operate import _upload_batch
    src = flat_source(data_loader)
    if src is not None:
        p3, p2 = src
        M, B = p3.shape[0], data_loader.batch_size
        perm = torch.randperm(M, device=p3.device)
        for i in range(0, M, B):
            yield ops.pair_batch(p3, p2, idx=perm[i:i + B], flip=flip, playback=playback)
        return
    for batch in data_loader:
        b3, b2 = pick(batch)
        if b3.shape[0] == 1:                 # the reference's loops stop at a batch of one pose
            return
        yield ops.pair_batch(_upload_batch(b3, device), _upload_batch(b2, device), flip=flip, playback=playback)


def summary_line(title, m):
    print("{}: {} steps | Loss: {: .4f} | flip_Loss: {: .4f} | back_Loss: {: .4f} | back_flip_Loss: {: .4f}"
          .format(title, m["steps"], m["loss"], m["flip_loss"], m["back_loss"], m["back_flip_loss"]))


def train_posenet(model_pos, data_loader, optimizer, criterion, device, args):
    torch.set_grad_enabled(True)
    set_grad([model_pos], True)
    model_pos.train()
    run = StepRunner(model_pos, optimizer, criterion, device)
    flip = bool(args.flip_pos_model_input)
    for b in pair_batches(data_loader, device, flip, False, lambda batch: (batch[0], batch[1])):
        num_poses = b["tgt"].shape[0]
        if num_poses == 1:
            break
        if b["tgt"].shape[1] != 1 or b["inp"].shape[1] != 1:
            raise ValueError("train_posenet: single-frame pairs expected, got %s and %s"
                             % (tuple(b["tgt"].shape), tuple(b["inp"].shape)))
        run.step(b["inp"].view(num_poses, 16, 2), b["tgt"].view(num_poses, 16, 3), "loss", num_poses)
        if flip:
            run.step(b["inp_flip"].view(num_poses, -1), b["tgt_flip"].view(num_poses, 16, 3), None, num_poses)   # (meter: finish())
    train_posenet.last_meters = run.finish(flip)
    train_posenet.last_trace = run.trace_tensor()
    summary_line("Train posenet", train_posenet.last_meters)
    return


train_posenet.last_meters = None
train_posenet.last_trace = None
