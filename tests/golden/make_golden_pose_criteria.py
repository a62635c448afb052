#!/usr/bin/env python3
"""Generate tests/golden/pose_criteria.npz by RUNNING THE REFERENCE's n_mpjpe, weighted_mpjpe and mpjpe_byjoint (utils/loss.py)
and its two video posenet training loops on the CPU (build container only: the reference is imported through
tests/golden/_ref_import.py, with its root on sys.path and as working directory; one thread).  Re-run with
    python tests/golden/make_golden_pose_criteria.py

Contents (shapes, weights and the restated formulas are tests/pose_criteria_util.py; the stub posenet, the data builder and the
loaders are tests/posetrain_util.py; the gain of the stub's last layer is tests/posetrain_mpjpe_util.py):
 (a) for k = 0, 1, 2 (pose_criteria_util.SHAPES):
  a<k>_pred / _target / _w_pose / _w_joint / _w16 / _cot      the fp32 inputs of pose_criteria_util.make_case(shape, 40 + k)
  a<k>_<c>_value / _grad     the reference's function on those inputs cast to fp64, and torch's autograd gradient with respect to
                             predicted: c = n (n_mpjpe), wp / wj / w16 (weighted_mpjpe with the per-pose weight, the per-joint
                             weight, the 16-vector expanded over the poses), bj (mpjpe_byjoint; _grad for the cotangent _cot)
 (b) for loop in {video, gan} = video_mode_train_posenet, GAN_dataSet_video_mode_train_posenet and c in {n, w16} = the
     reference's n_mpjpe, and lambda p, t: weighted_mpjpe(p, t, LOOP_W16.expand(p.shape[:-1])), as the criterion:
  init_<key>                            state_dict before the loop: the same for both loops and both criteria (asserted here).  The
                                        clips are posetrain_util.make_data()'s, stored as v_b3d / v_b2d in posetrain_mpjpe.npz
  <c>_<loop>_final_<key>                every parameter and buffer after the loop (Adam lr 1e-3, flip on, playback on: 12 steps)
  <c>_<loop>_losses / _norms            per optimizer step: the criterion's value and what clip_grad_norm_ returned
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
import pose_criteria_util as CU    # noqa: E402

torch.set_num_threads(1)


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from models_Fk_GAN import video_mode_operate as V
    from utils import loss as RL

    rec = {}
    # (a) values and autograd gradients of the reference's own functions, fp64
    for k, shape in enumerate(CU.SHAPES):
        case = CU.make_case(shape, 40 + k)
        t64 = {name: torch.from_numpy(a).double() for name, a in case.items()}
        for name, a in case.items():
            rec["a%d_%s" % (k, name)] = a
        calls = dict(n=lambda p: RL.n_mpjpe(p, t64["target"]),
                     wp=lambda p: RL.weighted_mpjpe(p, t64["target"], t64["w_pose"]),
                     wj=lambda p: RL.weighted_mpjpe(p, t64["target"], t64["w_joint"]),
                     w16=lambda p: RL.weighted_mpjpe(p, t64["target"], t64["w16"].expand(shape[:-1])),
                     bj=lambda p: RL.mpjpe_byjoint(p, t64["target"]))
        for c, fn in calls.items():
            p = t64["pred"].clone().requires_grad_(True)
            v = fn(p)
            (v * t64["cot"]).sum().backward() if c == "bj" else v.backward()
            rec["a%d_%s_value" % (k, c)] = v.detach().numpy().copy()
            rec["a%d_%s_grad" % (k, c)] = p.grad.numpy().copy()

    # (b) the two video loops with each criterion
    fns = dict(video=V.video_mode_train_posenet, gan=V.GAN_dataSet_video_mode_train_posenet)
    data = PU.make_data()
    clips = MU.load_golden()
    assert np.array_equal(clips["v_b3d"], data["v_b3d"]) and np.array_equal(clips["v_b2d"], data["v_b2d"])
    w16 = torch.from_numpy(CU.LOOP_W16)
    criteria = dict(n=RL.n_mpjpe, w16=lambda p, t: RL.weighted_mpjpe(p, t, w16.expand(p.shape[:-1])))
    clip, norms, values = nn.utils.clip_grad_norm_, [], []

    def recording_clip(*a, **k):
        r = clip(*a, **k)
        norms.append(float(r))
        return r

    nn.utils.clip_grad_norm_ = recording_clip
    try:
        for c in CU.CRITERIA:
            def recording(predicted, target, fn=criteria[c]):
                loss = fn(predicted, target)
                values.append(float(loss.item()))
                return loss

            for loop in CU.LOOPS:
                model = MU.make_model(loop)
                for k, t in model.state_dict().items():
                    assert np.array_equal(rec.setdefault("init_" + k, t.numpy().copy()), t.numpy())
                batches = PU.batches_of(data, loop)
                if loop == "video":                      # the reference's generator yields float64 numpy batches
                    batches = [(b3.double().numpy(), b2.double().numpy()) for b3, b2 in batches]
                del norms[:], values[:]
                fns[loop](model, PU.loader_of(loop, batches), torch.optim.Adam(model.parameters(), lr=PU.LR), recording,
                          torch.device("cpu"), PU.loop_args())
                for k, t in model.state_dict().items():
                    rec["%s_%s_final_%s" % (c, loop, k)] = t.numpy().copy()
                rec["%s_%s_losses" % (c, loop)], rec["%s_%s_norms" % (c, loop)] = np.array(values), np.array(norms)
                print(c, loop, len(norms), "steps, norms", " ".join("%.3f" % v for v in norms))
    finally:
        nn.utils.clip_grad_norm_ = clip
    np.savez_compressed(CU.GOLDEN, **rec)
    print("wrote", CU.GOLDEN, os.path.getsize(CU.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
