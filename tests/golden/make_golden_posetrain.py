#!/usr/bin/env python3
"""Generate tests/golden/posetrain.npz by RUNNING THE REFERENCE's three posenet training loops on the CPU (build container only:
the reference is imported through tests/golden/_ref_import.py, with its root on sys.path and as working directory; one thread).
Re-run with
    python tests/golden/make_golden_posetrain.py

Contents (the stub posenet, the data builder and the loaders are tests/posetrain_util.py):
  s_t3d / s_i2d                 single-frame pairs (520 poses: batches of 96 and a last one of 40)
  v_b3d / v_b2d                 clips (160: batches of 64, 64, 32), one 3D frame and posetrain_util.FRAMES 2D frames each
  <loop>_init_<key>             state_dict before the loop, loop in {single, video, gan} = train_posenet,
                                video_mode_train_posenet, GAN_dataSet_video_mode_train_posenet
  <loop>_final_<key>            every parameter and buffer after the loop (Adam lr 1e-3, flip on, playback on)
  <loop>_losses / _norms        per optimizer step: the value of the criterion and what clip_grad_norm_ returned, captured by
                                wrapping those two calls
  sig_<function>                the reference signatures
"""
import inspect
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI     # noqa: E402
import posetrain_util as PU  # noqa: E402

torch.set_num_threads(1)


class RecordingCriterion(nn.Module):
    def __init__(self):
        super().__init__()
        self.inner, self.values = nn.MSELoss(reduction='mean'), []

    def forward(self, a, b):
        loss = self.inner(a, b)
        self.values.append(float(loss.item()))
        return loss


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from function_aug import model_pos_train as MT
    from models_Fk_GAN import video_mode_operate as V

    fns = dict(single=MT.train_posenet, video=V.video_mode_train_posenet, gan=V.GAN_dataSet_video_mode_train_posenet)
    rec = dict(PU.make_data())
    clip, norms = nn.utils.clip_grad_norm_, []

    def recording_clip(*a, **k):
        r = clip(*a, **k)
        norms.append(float(r))
        return r

    nn.utils.clip_grad_norm_ = recording_clip
    try:
        for loop in PU.LOOPS:
            model = PU.make_model(loop)
            for k, t in model.state_dict().items():
                rec["%s_init_%s" % (loop, k)] = t.numpy().copy()
            batches = PU.batches_of(rec, loop)
            if loop == "video":                      # the reference's generator yields float64 numpy batches
                batches = [(b3.double().numpy(), b2.double().numpy()) for b3, b2 in batches]
            crit = RecordingCriterion()
            del norms[:]
            fns[loop](model, PU.loader_of(loop, batches), torch.optim.Adam(model.parameters(), lr=PU.LR), crit,
                      torch.device("cpu"), PU.loop_args())
            for k, t in model.state_dict().items():
                rec["%s_final_%s" % (loop, k)] = t.numpy().copy()
            rec[loop + "_losses"], rec[loop + "_norms"] = np.array(crit.values), np.array(norms)
            print(loop, len(norms), "steps, norms %.3f .. %.3f" % (min(norms), max(norms)))
    finally:
        nn.utils.clip_grad_norm_ = clip
    names = dict(single="train_posenet", video="video_mode_train_posenet", gan="GAN_dataSet_video_mode_train_posenet")
    for loop, f in fns.items():
        rec["sig_" + names[loop]] = np.array([str(inspect.signature(f))])
    out = os.path.join(HERE, "posetrain.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
