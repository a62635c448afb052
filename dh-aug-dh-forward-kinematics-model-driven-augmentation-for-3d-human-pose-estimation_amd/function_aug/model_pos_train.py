"""Drop-in for the posenet training loop of R/function_aug/model_pos_train.py (train_posenet :13-83), and the step machinery
the video loops of models_Fk_GAN/video_mode_operate.py share with it.

The posenet is whatever nn.Module the caller passes; what runs in this package's kernels is everything around its call:
  * the batch: one dhaug_pair_batch launch makes the root-centred targets, the inputs and their flipped / frame-reversed copies
    (for FakePairBuffer / TensorLoader sources from ONE permutation per epoch and index slices, for any other loader after the
    upload);
  * nn.MSELoss(reduction='mean'): dhaug_pose_mse gives the loss, its gradient (the loop calls outputs.backward(grad)) and the
    epoch's loss meter, AverageMeter.update(loss, num_poses) on the device;
  * utils.loss.mpjpe of this package (the criterion of the reference's video command): dhaug_pose_mpjpe, the same way;
  * utils.loss.n_mpjpe and any utils.loss.JointWeightedMpjpe instance: dhaug_pose_nmpjpe / dhaug_pose_wmpjpe, the same way;
  * nn.utils.clip_grad_norm_(max_norm=1) + optimizer.step(): optimizer.clip_step(1) of optim.PosenetAdam, two launches.
Each piece falls back on its own to what the reference calls (criterion(...).backward(), clip_grad_norm_, optimizer.step() of a
stock torch optimizer) when it does not apply; the loss still goes to the meter on the device.  Nothing is read on the host per
batch: the meters are read once when the loop ends and one summary line replaces the progress bar.  The loops return None as
the reference's do; the epoch's averages stay on <function>.last_meters, the per-step losses and gradient norms (device
tensors, never read here) on <function>.last_trace.

graph=True (StepRunner's argument; the loops pass it for args.posenet_graph or DHAUG_POSENET_GRAPH=1) replays the step as a
hipGraph: a step is 110-160 launches of a few microseconds, so issued one by one it is bound by the host.  What makes it replayable:
the dropout masks' Philox position lives on the device (autograd_ops.DeviceDropoutStream, the _dr BatchNorm entries), the learning
rate is read from a device float (dhaug_adam_clip_step_lr), and the host bookkeeping a replay skips is done behind it
(PosenetAdam.note_step, the model's _stat_epoch).  See StepRunner."""
import os
import warnings

import torch
import torch.nn as nn

from .. import autograd_ops as A
from .. import ops
from ..optim import PosenetAdam
from ..utils.loss import JointWeightedMpjpe, mpjpe, n_mpjpe

METERS = ("loss", "flip_loss", "back_loss", "back_flip_loss")
# DHAUG_POSENET_GRAPH=1: the three loops replay the posenet step as a hipGraph without being asked through args (read once, here)
POSENET_GRAPH = os.environ.get("DHAUG_POSENET_GRAPH", "") in ("1", "true", "yes")
_TRACE_CHUNK = 1024


def posenet_optimizer(model_pos, lr=1e-3):
    """the optimizer of the reference's posenet (torch.optim.Adam(model_pos.parameters(), lr)) on flat buffers, with clip_step"""
    return PosenetAdam(model_pos.parameters(), lr=lr)


def set_grad(nets, requires_grad=False):
    for net in nets:
        for p in net.parameters():
            p.requires_grad = requires_grad


def graph_requested(args):
    """what the three loops pass as StepRunner's graph: args.posenet_graph, or DHAUG_POSENET_GRAPH=1; off by default"""
    return bool(getattr(args, "posenet_graph", False)) or POSENET_GRAPH


def fused_criterion(criterion):
    """the name of the fused loss + gradient launch pair a criterion stands for, or None (the generic path: criterion(outputs,
    targets).backward()).  Four are fused: nn.MSELoss(reduction='mean') -> "mse", and of this package's utils.loss the functions
    mpjpe -> "mpjpe" and n_mpjpe -> "n_mpjpe" themselves (identity, not equality of results) and any JointWeightedMpjpe instance
    -> "wmpjpe".  Decided from the object alone, before any GPU work."""
    if isinstance(criterion, nn.MSELoss):
        return "mse" if criterion.reduction == "mean" else None
    if criterion is mpjpe:
        return "mpjpe"
    if criterion is n_mpjpe:
        return "n_mpjpe"
    if isinstance(criterion, JointWeightedMpjpe):
        return "wmpjpe"
    return None


def _graph_models():
    from ..models_baseline.gcn.sem_gcn import SemGCN
    from ..models_baseline.mlp.linear_model import LinearModel
    from ..models_baseline.videopose.model_VideoPose3D import TemporalModelOptimized1f
    from ..models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModelOptimized1f
    return (TemporalModelOptimized1f, LinearModel, multiFrame_TemporalModelOptimized1f, SemGCN)


class _CapturedStep:
    """one key's hipGraph with its static inputs and the dropout calls one replay stands for"""
    __slots__ = ("graph", "inputs", "targets", "dropout_calls")


class GraphState:
    """What the captured steps of one optimizer share.  It lives ON the optimizer (optimizer._dhaug_graph_state): a StepRunner lives
    for one epoch, the graphs for the whole run.  rng_cell {seed, base} and lr_cell are what the captured kernels read in place of
    launch immediates; out = (loss, norm), the meters and the loss workspace are written by them (fixed addresses); steps maps a key
    to [sightings, _CapturedStep | None, capture failed]."""

    def __init__(self, device):
        self.rng_cell = torch.zeros(2, dtype=torch.int64, device=device)
        self.dropout = A.DeviceDropoutStream(self.rng_cell)
        self.lr_cell = torch.zeros(1, dtype=torch.float32, device=device)
        self.lr = None                                # the value lr_cell holds
        self.out = torch.zeros(2, dtype=torch.float32, device=device)
        self.meters = ops.loss_meters(len(METERS), device)
        self.workspace = ops.posetrain_workspace(device)
        self.steps = {}
        self.captures = 0

    def seed(self, gen):
        """the stream starts where the torch generator stands; returns that offset"""
        seed, off = gen.initial_seed(), gen.get_offset()
        words = [w - (1 << 64) if w >= (1 << 63) else w for w in (seed & 0xFFFFFFFFFFFFFFFF, off)]
        self.rng_cell.copy_(torch.tensor(words, dtype=torch.int64))
        return off

    def set_lr(self, lr):
        """one fill, and only when the schedule moved"""
        if lr != self.lr:
            self.lr_cell.fill_(lr)
            self.lr = lr


class StepRunner:
    """One epoch's training steps.  step(inputs, targets, meter) = the reference's

        outputs = model_pos(inputs); optimizer.zero_grad(); loss = criterion(outputs, targets); loss.backward()
        nn.utils.clip_grad_norm_(model_pos.parameters(), max_norm=1); optimizer.step(); meter.update(loss.item(), num_poses)

    with the loss, the meter and the norm kept on the device.

    graph=True: the step is captured per key (input shape, target shape, meter, model class, precision, criterion, num_poses and
    the layers' launch immediates: dropout rates, BatchNorm momenta and eps) and replayed.  The first two steps of a key run
    launch by launch through the device dropout stream and the lr cell -- real training steps, and the capture's warm-up; at the
    third sighting the step is captured on graphs.capture_streams()'s capture stream (autograd_ops.CAPTURE_ID set: the weights'
    operand copies are rebuilt inside the graph) and replayed at once.  A replay copies inputs and targets into the graph's
    buffers, refreshes the lr cell if param_groups[0]['lr'] moved, replays, copies (loss, norm) into the trace row and does the
    host bookkeeping of the optimizer and the model.  A capture that raises is ended, the key stays eager for good (one warning).
    The masks are the eager path's: the stream is seeded from the torch generator at the runner's first step, and finish() moves
    the generator past the calls the stream handed out (counted on the host).  eager_steps, replayed_steps, captures count."""

    def __init__(self, model_pos, optimizer, criterion, device, graph=False):
        self.model, self.opt, self.criterion = model_pos, optimizer, criterion
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the posenet training loops need a GPU (no CPU fallback exists)")
        self.graph = bool(graph)
        self.eager_steps = self.replayed_steps = 0
        if self.graph:
            self._check_graph_support()
        # the fused criteria (fused_criterion); any other callable is called as it is
        self.fused = fused_criterion(criterion)
        self.fused_opt = hasattr(optimizer, "clip_step")
        self.state = None
        if self.graph:
            st = getattr(optimizer, "_dhaug_graph_state", None)
            if st is None:
                st = optimizer._dhaug_graph_state = GraphState(self.device)
            self.state = st
            st.meters.zero_()           # the captured steps write THESE meters: a new epoch starts them again
            self.meters, self.workspace = st.meters, st.workspace
            self._gen = torch.cuda.default_generators[self.device.index if self.device.index is not None
                                                      else torch.cuda.current_device()]
            self._seeded = False
            self._credited = st.dropout.calls     # the stream's count up to which the torch generator has been moved along
        else:
            self.meters = ops.loss_meters(len(METERS), self.device)
            self.workspace = ops.posetrain_workspace(self.device)
        self.trace = []                 # (chunk, 2) fp32 device tensors: loss and gradient norm of every step
        self.steps = 0

    @property
    def captures(self):
        """graphs captured for this optimizer so far, by this runner or an earlier one"""
        return 0 if self.state is None else self.state.captures

    def _check_graph_support(self):
        """graph=True refusals: before any GPU work, with no capture begun"""
        if not hasattr(self.opt, "clip_step"):
            raise ValueError("StepRunner(graph=True) needs an optimizer with clip_step (posenet_optimizer / optim.PosenetAdam), got %s"
                             % type(self.opt).__name__)
        if fused_criterion(self.criterion) is None:
            raise ValueError("StepRunner(graph=True) captures the four fused criteria only: nn.MSELoss(reduction='mean') and this "
                             "package's utils.loss.mpjpe, utils.loss.n_mpjpe and utils.loss.JointWeightedMpjpe instances, got %r"
                             % (self.criterion,))
        if self.opt.world_size() > 1:
            raise NotImplementedError("StepRunner(graph=True) with a world size above 1: a captured step cannot hold the gradient "
                                      "all-reduce (segmented graphs around the collective are not implemented)")
        if not isinstance(self.model, _graph_models()):
            raise NotImplementedError("StepRunner(graph=True) supports %s, got %s%s" % (
                ", ".join(t.__name__ for t in _graph_models()), type(self.model).__name__,
                " (its drop path and attention path draw their masks on the host)"
                if type(self.model).__name__ == "PoseTransformer" else ""))

    def _slot(self):
        k = self.steps % _TRACE_CHUNK
        if k == 0:
            self.trace.append(torch.zeros((_TRACE_CHUNK, 2), dtype=torch.float32, device=self.device))
        self.steps += 1
        return self.trace[-1][k]

    def step(self, inputs, targets, meter, num_poses):
        if self.graph and not self.model.training:
            raise RuntimeError("StepRunner(graph=True).step: the model is not in training mode (call model.train() first)")
        row = self._slot()
        if self.graph:
            return self._graph_step(inputs, targets, meter, num_poses, row)
        self.eager_steps += 1
        self._body(inputs, targets, meter, num_poses, row[0:1], row[1:2], None)

    def _fused_loss(self, outputs, targets, num_poses, rec, loss_slot):
        """(loss, grad) of the fused criterion from one launch pair, the meter record updated on the device"""
        kw = dict(meter=rec, workspace=self.workspace, loss=loss_slot)
        if self.fused == "mse":
            return ops.pose_mse(outputs, targets, num_poses, **kw)
        if self.fused == "mpjpe":
            return ops.pose_mpjpe(outputs, targets, num_poses, **kw)
        if self.fused == "n_mpjpe":
            if outputs.dim() != 4:                # what utils.loss.n_mpjpe raises
                raise ValueError("n_mpjpe: poses must be (B, F, 16, 3), got %s" % (tuple(outputs.shape),))
            return ops.pose_nmpjpe(outputs, targets, num_poses, **kw)
        return ops.pose_wmpjpe(outputs, targets, self.criterion.buffer(outputs.device), num_poses, **kw)

    def _body(self, inputs, targets, meter, num_poses, loss_slot, norm_slot, lr_dev):
        rec = None if meter is None else self.meters[METERS.index(meter)]
        outputs = self.model(inputs)
        self.opt.zero_grad()
        if self.fused is not None:
            if tuple(outputs.shape) != tuple(targets.shape):
                raise ValueError("posenet output %s and target %s differ in shape" % (tuple(outputs.shape), tuple(targets.shape)))
            _, grad = self._fused_loss(outputs, targets, num_poses, rec, loss_slot)
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
        if lr_dev is not None:
            self.opt.clip_step(1, norm_out=norm_slot, lr_dev=lr_dev)
        elif self.fused_opt:
            self.opt.clip_step(1, norm_out=norm_slot)
        else:
            norm = nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=1)
            self.opt.step()
            norm_slot.copy_(norm.detach().reshape(1))

    # ------------------------------------------------------------------------------------------------ graph=True
    def _key(self, inputs, targets, meter, num_poses):
        imm = []
        for m in self.model.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                imm.append((m.momentum, m.eps))
            elif isinstance(m, nn.Dropout):
                imm.append(m.p)
        # the weighted criterion's captured launch reads the weight buffer in place: another buffer is another graph
        crit = (self.fused, self.criterion.buffer(self.device).data_ptr()) if self.fused == "wmpjpe" else self.fused
        return (tuple(inputs.shape), tuple(targets.shape), -1 if meter is None else METERS.index(meter), type(self.model),
                self.model.precision, crit, int(num_poses), tuple(imm))

    def _graph_step(self, inputs, targets, meter, num_poses, row):
        st = self.state
        if not self._seeded:
            st.seed(self._gen)
            self._seeded = True
        st.set_lr(self.opt.param_groups[0]["lr"])
        ent = st.steps.setdefault(self._key(inputs, targets, meter, num_poses), [0, None, False])
        ent[0] += 1
        if ent[1] is None and not ent[2] and ent[0] >= 3:
            self._capture(ent, inputs, targets, meter, num_poses)
        if ent[1] is not None:
            self._replay(ent[1], inputs, targets, row)
        else:
            self._device_stream_step(inputs, targets, meter, num_poses, row[0:1], row[1:2])
            self.eager_steps += 1

    def _device_stream_step(self, inputs, targets, meter, num_poses, loss_slot, norm_slot):
        """the step launch by launch, masks from the device stream, lr from the cell; the base moves behind the backward pass"""
        st = self.state
        A.DEVICE_DROPOUT = st.dropout
        try:
            self._body(inputs, targets, meter, num_poses, loss_slot, norm_slot, st.lr_cell)
            return st.dropout.advance()
        finally:
            A.DEVICE_DROPOUT = None
            st.dropout.k = 0

    def _capture(self, ent, inputs, targets, meter, num_poses):
        from .. import graphs
        st = self.state
        cs = _CapturedStep()
        cs.inputs, cs.targets = inputs.detach().clone(), targets.detach().clone()
        cs.graph = torch.cuda.CUDAGraph()
        _, cap = graphs.capture_streams()
        # capturing runs the host side of a step without running the step: what it bumps is put back (the replay behind it bumps it)
        host = (self.opt.step_count, self.model._stat_epoch, st.dropout.calls)
        cur = torch.cuda.current_stream()
        A.CAPTURE_ID = next(graphs._capture_ids)
        ops.ZERO_BY_KERNEL = True                       # no memset nodes in the graph: see ops.ZERO_BY_KERNEL
        try:
            with torch.cuda.graph(cs.graph, stream=cap):
                cs.dropout_calls = self._device_stream_step(cs.inputs, cs.targets, meter, num_poses, st.out[0:1], st.out[1:2])
            ent[1] = cs
            st.captures += 1
        except Exception as e:                          # (torch.cuda.graph has ended the capture on its way out)
            ent[2] = True
            torch.cuda.set_stream(cur)
            warnings.warn("StepRunner(graph=True): capturing the step of %s failed (%s: %s); this shape stays on the eager path"
                          % (type(self.model).__name__, type(e).__name__, e))
        finally:
            A.CAPTURE_ID = 0
            ops.ZERO_BY_KERNEL = False
            self.opt.step_count, self.model._stat_epoch, st.dropout.calls = host

    def _replay(self, cs, inputs, targets, row):
        cs.inputs.copy_(inputs, non_blocking=True)
        cs.targets.copy_(targets, non_blocking=True)
        cs.graph.replay()
        row.copy_(self.state.out, non_blocking=True)
        # what a replay skips on the host: the optimizer's (stale packed copies, step_count, _opt_called) and the model's (an eager
        # training forward advances _stat_epoch, which the evaluation caches compare)
        self.opt.note_step()
        self.model._stat_epoch += 1
        self.state.dropout.calls += cs.dropout_calls
        self.replayed_steps += 1

    def finish(self, flip):
        """the one host read: the meters' averages as a dict; the trace stays on the device.  graph=True: the torch generator is
        moved past the dropout calls of this runner's steps, 4 per call as autograd_ops.dropout_stream does on the eager path (from
        the host's count; the device is not read for it).  With nothing else drawing from the generator during the epoch that is
        start + 4 x calls, start being where the stream was seeded; a draw in between keeps its own advance"""
        if self.graph and self._seeded:
            calls = self.state.dropout.calls
            self._gen.set_offset(self._gen.get_offset() + 4 * (calls - self._credited))
            self._credited = calls
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
    run = StepRunner(model_pos, optimizer, criterion, device, graph=graph_requested(args))
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
