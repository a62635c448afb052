"""Records tests/golden/ik_staged.npz: the fp64 restatement of the staged inverse-kinematics fit (tests/ik_staged_util.py) on the
first 256 poses of ik_util.trial_fit_inputs(256) (seed 20261021), cold from the T-pose with the coarse-to-fine schedule
(8 + 8 + 8 + 16 steps).  CPU only, about a minute:

    python tests/golden/make_ik_staged.py

    err         (256,) float64   largest joint distance per pose, metres (fp64 oracle FK of the fp64 solution)
    not_converged  int           R: poses with err > CONVERGED_M (1e-4 m)
    single_err  (256,) float64   the same from ik_util.lm_fit, one stage of 40 steps: what the schedule is measured against
    schedule_w  (4,16), schedule_iters (4,): the schedule that was run"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ik_util as K                   # noqa: E402
import ik_staged_util as KS           # noqa: E402


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    N = KS.GOLDEN_POSES
    err = KS.cold_errors(N)
    pose = KS.golden_inputs(N)
    single = K.joint_error(*K.lm_fit(pose, None, iters=40)[:3], pose)
    R = K.not_converged(err)
    print("staged: %d of %d not converged (first 128: %d), worst %.3g m; single stage of 40 steps: %d"
          % (R, N, K.not_converged(err[:128]), err.max().item(), K.not_converged(single)))
    np.savez(KS.GOLDEN, err=err.numpy(), not_converged=np.int64(R), single_err=single.numpy(),
             schedule_w=np.array([w for w, _ in KS.COARSE_TO_FINE], dtype=np.float64),
             schedule_iters=np.array([n for _, n in KS.COARSE_TO_FINE], dtype=np.int64))


if __name__ == "__main__":
    main()
