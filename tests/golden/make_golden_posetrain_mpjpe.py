#!/usr/bin/env python3
"""Generate tests/golden/posetrain_mpjpe.npz by RUNNING THE REFERENCE's two video posenet training loops on the CPU with the
reference's own utils.loss.mpjpe as the criterion -- what its video command passes (build container only: the reference is
imported through tests/golden/_ref_import.py, with its root on sys.path and as working directory; one thread).  Re-run with
    python tests/golden/make_golden_posetrain_mpjpe.py

Contents (the stub posenet, the data builder and the loaders are tests/posetrain_util.py; the gain of the stub's last layer is
tests/posetrain_mpjpe_util.py):
  v_b3d / v_b2d                 clips (160: batches of 64, 64, 32), one 3D frame and posetrain_util.FRAMES 2D frames each
  <loop>_init_<key>             state_dict before the loop, loop in {video, gan} = video_mode_train_posenet,
                                GAN_dataSet_video_mode_train_posenet
  <loop>_final_<key>            every parameter and buffer after the loop (Adam lr 1e-3, flip on, playback on: 12 steps)
  <loop>_losses / _norms        per optimizer step: the value of the criterion and what clip_grad_norm_ returned, captured by
                                wrapping those two calls
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI           # noqa: E402
import posetrain_util as PU        # noqa: E402
import posetrain_mpjpe_util as MU  # noqa: E402

torch.set_num_threads(1)


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from models_Fk_GAN import video_mode_operate as V
    from utils.loss import mpjpe as ref_mpjpe

    fns = dict(video=V.video_mode_train_posenet, gan=V.GAN_dataSet_video_mode_train_posenet)
    data = PU.make_data()
    rec = dict(v_b3d=data["v_b3d"], v_b2d=data["v_b2d"])
    clip, norms, values = nn.utils.clip_grad_norm_, [], []

    def recording_clip(*a, **k):
        r = clip(*a, **k)
        norms.append(float(r))
        return r

    def recording_mpjpe(predicted, target):
        loss = ref_mpjpe(predicted, target)
        values.append(float(loss.item()))
        return loss

    nn.utils.clip_grad_norm_ = recording_clip
    try:
        for loop in MU.LOOPS:
            model = MU.make_model(loop)
            for k, t in model.state_dict().items():
                rec["%s_init_%s" % (loop, k)] = t.numpy().copy()
            batches = PU.batches_of(rec, loop)
            if loop == "video":                      # the reference's generator yields float64 numpy batches
                batches = [(b3.double().numpy(), b2.double().numpy()) for b3, b2 in batches]
            del norms[:], values[:]
            fns[loop](model, PU.loader_of(loop, batches), torch.optim.Adam(model.parameters(), lr=PU.LR), recording_mpjpe,
                      torch.device("cpu"), PU.loop_args())
            for k, t in model.state_dict().items():
                rec["%s_final_%s" % (loop, k)] = t.numpy().copy()
            rec[loop + "_losses"], rec[loop + "_norms"] = np.array(values), np.array(norms)
            print(loop, len(norms), "steps, norms", " ".join("%.3f" % v for v in norms))
    finally:
        nn.utils.clip_grad_norm_ = clip
    np.savez_compressed(MU.GOLDEN, **rec)
    print("wrote", MU.GOLDEN, os.path.getsize(MU.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
