#!/usr/bin/env python3
"""Generate tests/golden/posenet_multiframe.npz by RUNNING THE REFERENCE's multiFrame_TemporalModelOptimized1f (the strided training
model), multiFrame_TemporalModel (the dilated evaluation model) and video_mode_train_posenet on the CPU (build container only: the
reference is imported through tests/golden/_ref_import.py; one thread).  Re-run with
    python tests/golden/make_golden_multiframe.py

Weights and inputs are regenerated from seeds by both sides (tests/multiframe_util.py) and are not stored.  Dropout is 0 everywhere.
The yardstick is the reference class converted with .double() (see make_golden_posenet.py for why).
  keys_<arch> / shapes_<arch> / dtypes_<arch>    the state_dict layout of both reference classes (checked to be the same) at 1 024
                                                 channels, arch = 33 and 333
  a<B>_*  (C = 64, '3,3', B = 8, 5)              whole tensors of the strided class: out (training mode), loss, grad_<key>,
                                                 buf_<key> (BatchNorm buffers after the forward), eval_out (evaluation-mode output
                                                 on the training input after it); B = 5 makes the row counts ragged
          dil_out                                the dilated class's evaluation output on a (2, 9 + 7, 16, 2) input, its state the
                                                 seeded one with the running buffers set from the seed
  a27_<B>_* (C = 64, '3,3,3', B = 4)             the same
  b_*  (C = 1 024, '3,3', B = 8)                 the same through golden_util.compact records (<name>__full | __sample, __proj)
  c_final_<key>, c_losses, c_norms               the reference's video_mode_train_posenet with its own strided class (C = 64, '3,3'):
                                                 160 clips of 9 frames, batches 64, 64, 32, flip and playback on, Adam lr 1e-3: the
                                                 state after the 12 steps, the criterion's value and clip_grad_norm_'s result per step"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI       # noqa: E402
import golden_util as GU       # noqa: E402
import multiframe_util as MU   # noqa: E402
import posetrain_util as PU    # noqa: E402

torch.set_num_threads(1)


def run(Strided, Dilated, cfg, B):
    arch = list(cfg["arch"])
    model = Strided(16, 2, 16, filter_widths=arch, causal=False, dropout=0.0, channels=cfg["C"])
    model.load_state_dict(MU.seeded_state(cfg["C"], cfg["arch"], cfg["seed"]), strict=True)
    model = model.double()
    x, t = MU.record_inputs(cfg, B)
    x, t = x.double(), t.double()
    model.train()
    out = model(x)
    loss = nn.functional.mse_loss(out, t)
    loss.backward()
    rec = dict(out=out.detach(), loss=loss.detach().reshape(1))
    for k, p in model.named_parameters():
        rec["grad_" + k] = p.grad.detach()
    for k, b in model.named_buffers():
        rec["buf_" + k] = b.detach().clone()
    model.eval()
    with torch.no_grad():
        rec["eval_out"] = model(x)
    dil = Dilated(16, 2, 16, filter_widths=arch, causal=False, dropout=0.0, channels=cfg["C"])
    dil.load_state_dict(MU.seeded_state(cfg["C"], cfg["arch"], cfg["seed"], running=True), strict=True)
    dil = dil.double().eval()
    with torch.no_grad():
        rec["dil_out"] = dil(MU.dilated_input(cfg).double())
    return rec


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModel as Dilated
    from models_Fk_GAN.mulit_farme_videopose import multiFrame_TemporalModelOptimized1f as Strided
    from models_Fk_GAN import video_mode_operate as V

    out = {}
    for arch in MU.LAYOUTS:
        sds = [cls(16, 2, 16, filter_widths=list(arch), causal=False, dropout=0.25, channels=1024).state_dict()
               for cls in (Strided, Dilated)]
        lay = [(list(sd.keys()), [",".join(str(d) for d in v.shape) for v in sd.values()], [str(v.dtype) for v in sd.values()])
               for sd in sds]
        assert lay[0] == lay[1], "the two reference classes differ in their state_dict layout"
        out["keys_" + MU.tag(arch)], out["shapes_" + MU.tag(arch)], out["dtypes_" + MU.tag(arch)] = (np.array(v) for v in lay[0])

    for B in MU.BATCH_A:
        for k, v in run(Strided, Dilated, MU.SMALL, B).items():
            out["a%d_%s" % (B, k)] = v.numpy()
    for k, v in run(Strided, Dilated, MU.SMALL27, MU.BATCH_A27).items():
        out["a27_%d_%s" % (MU.BATCH_A27, k)] = v.numpy()
    for i, (k, v) in enumerate(run(Strided, Dilated, MU.WIDE, MU.BATCH_B).items()):
        if v.dtype.is_floating_point:
            for part, a in GU.compact(v, i).items():
                out["b_%s__%s" % (k, part)] = a.numpy()
        else:
            out["b_" + k] = v.numpy()

    # (c): the reference's video loop with its own strided class; its generators yield float64 numpy batches
    cfg = MU.SMALL
    model = Strided(16, 2, 16, filter_widths=list(cfg["arch"]), causal=False, dropout=0.0, channels=cfg["C"])
    model.load_state_dict(MU.seeded_state(cfg["C"], cfg["arch"], cfg["seed"]), strict=True)
    batches = [(b3.double().numpy(), b2.double().numpy()) for b3, b2 in MU.train_batches()]
    clip, norms, losses = nn.utils.clip_grad_norm_, [], []

    class Crit(nn.Module):
        def forward(self, a, b):
            loss = nn.functional.mse_loss(a, b)
            losses.append(float(loss.item()))
            return loss

    def recording_clip(*a, **k):
        r = clip(*a, **k)
        norms.append(float(r))
        return r

    nn.utils.clip_grad_norm_ = recording_clip
    try:
        V.video_mode_train_posenet(model, PU.loader_of("video", batches), torch.optim.Adam(model.parameters(), lr=MU.TRAIN["lr"]),
                                   Crit(), torch.device("cpu"), PU.loop_args())
    finally:
        nn.utils.clip_grad_norm_ = clip
    for k, v in model.state_dict().items():
        out["c_final_" + k] = v.numpy().copy()
    out["c_losses"], out["c_norms"] = np.array(losses), np.array(norms)
    print("loop:", len(norms), "steps, norms %.3f .. %.3f, loss %.4f -> %.4f" % (min(norms), max(norms), losses[0], losses[-1]))

    np.savez_compressed(MU.GOLDEN, **out)
    print("wrote", MU.GOLDEN, os.path.getsize(MU.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
