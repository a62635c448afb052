#!/usr/bin/env python3
"""Generate tests/golden/pose_eval.npz by RUNNING THE REFERENCE's posenet evaluation on the CPU (build container only: the
reference is imported through tests/golden/_ref_import.py, with its root on sys.path and as working directory).  Re-run with
    python tests/golden/make_golden_eval.py

Contents (inputs are stored; the stubs and case builders are tests/eval_util.py):
  m_<case>_pred / _target          metric cases (eval_util.metric_cases), fp32 (n, 16, 3)
  m_<case>_pp32 / _pp64            p_mpjpe per pose, on the fp32 inputs and on them cast to fp64
  m_<case>_p2, _p1                 p_mpjpe of the whole case (fp32), mpjpe (torch fp32)
  m_<case>_pck, _pcks, _auc        compute_PCK at 150, compute_PCK at each of the 31 AUC thresholds, compute_AUC
  m_<case>_pck_ej, _auc_ej         the same two with eval_joints = eval_util.EVAL_JOINTS
  z_pred / z_target / z_pp64       the zero-spread case: NaN per pose where the reference's 0 / 0 makes numpy's SVD
                                   raise (z_raised = 1 there)
  e_<set>_t3d / _i2d               evaluate sets (1 000 and 700 poses, batches of 256), w1 b1 w2 b2 the MLP posenet
  e_<set>_<flip>_<pck>             evaluate's returned tuple, flip in {noflip, flip}, pck in {0, 1}
  w_names / w_values / w_steps     writer scalars of evaluate_posenet (s1000 as H36M, s700 as 3DHP, epoch 7, tag '_real')
  ep_result                        evaluate_posenet's returned tuple
  v_b3d / v_b2d / v_sizes          batches of the reference ChunkedGenerator (architecture 3,3, batch 64), vw vb the posenet
  v_noflip / v_flip                video_mode_evaluate's returned tuples (get_pck_auc True)
  sig_<function>                   the reference signatures (argument names and defaults)
"""
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI     # noqa: E402
import eval_util as EU       # noqa: E402

torch.set_num_threads(1)


def sig(f):
    return np.array([str(inspect.signature(f))])


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from utils import loss as L
    from function_aug import model_pos_eval as ME
    from models_Fk_GAN import video_mode_operate as V

    rec = {}
    for name, (y, x) in EU.metric_cases().items():
        k = "m_" + name
        rec[k + "_pred"], rec[k + "_target"] = y, x
        rec[k + "_pp32"] = np.array([L.p_mpjpe(y[i:i + 1], x[i:i + 1]) for i in range(len(y))], dtype=np.float32)
        rec[k + "_pp64"] = np.array([L.p_mpjpe(y[i:i + 1].astype(np.float64), x[i:i + 1].astype(np.float64))
                                     for i in range(len(y))])
        rec[k + "_p2"] = np.array(L.p_mpjpe(y, x))
        rec[k + "_p1"] = L.mpjpe(torch.from_numpy(y), torch.from_numpy(x)).numpy()
        rec[k + "_pck"] = np.array(L.compute_PCK(x, y))
        rec[k + "_pcks"] = np.array([L.compute_PCK(x, y, threshold=t) for t in np.linspace(0, 150, 31)])
        rec[k + "_auc"] = np.array(L.compute_AUC(x, y))
        rec[k + "_pck_ej"] = np.array(L.compute_PCK(x, y, eval_joints=EU.EVAL_JOINTS))
        rec[k + "_auc_ej"] = np.array(L.compute_AUC(x, y, eval_joints=EU.EVAL_JOINTS))
    y, x = EU.zero_spread_case()
    rec["z_pred"], rec["z_target"] = y, x
    # the reference divides 0 / 0 there; numpy's SVD then raises on the NaN matrix: recorded as NaN (z_raised = 1)
    zp, zr = [], []
    for i in range(len(y)):
        try:
            with np.errstate(all="ignore"):
                zp.append(L.p_mpjpe(y[i:i + 1].astype(np.float64), x[i:i + 1].astype(np.float64)))
            zr.append(0)
        except np.linalg.LinAlgError:
            zp.append(np.nan)
            zr.append(1)
    rec["z_pp64"], rec["z_raised"] = np.array(zp), np.array(zr, dtype=np.int32)

    w = EU.posenet_weights()
    rec.update(w)
    net = EU.StubPosenet(w)
    loaders = {}
    for s, (n, seed) in EU.SETS.items():
        t3, i2 = EU.eval_set(n, seed)
        rec["e_%s_t3d" % s], rec["e_%s_i2d" % s] = t3, i2
        ds = torch.utils.data.TensorDataset(torch.from_numpy(t3), torch.from_numpy(i2))
        loaders[s] = torch.utils.data.DataLoader(ds, batch_size=EU.BATCH, shuffle=False)
        for flip in ("", "_flip"):
            for pck in (False, True):
                r = ME.evaluate(loaders[s], net, torch.device("cpu"), flipaug=flip, get_pck_auc=pck)
                rec["e_%s_%s_%d" % (s, "flip" if flip else "noflip", pck)] = np.array(r, dtype=np.float64)
    writer = EU.Writer()
    r = ME.evaluate_posenet(None, {"H36M_test": loaders["s1000"], "mpi3d_loader": loaders["s700"]}, net, EU.StubPosenet(w),
                            torch.device("cpu"), EU.Summary(7), writer, "_real", get_pck_auc=True)
    rec["ep_result"] = np.array(r, dtype=np.float64)
    rec["w_names"] = np.array([a for a, _, _ in writer.scalars])
    rec["w_values"] = np.array([b for _, b, _ in writer.scalars])
    rec["w_steps"] = np.array([c for _, _, c in writer.scalars])

    frames = int(np.prod([int(v) for v in EU.VIDEO_ARCH.split(",")]))
    vw = EU.video_weights(frames)
    rec.update(vw)
    p3, p2 = EU.video_sequences()
    gen = V.ChunkedGenerator(64, None, p3, p2, 1, pad=frames // 2, causal_shift=0, shuffle=False, augment=False)
    b3, b2, sizes = [], [], []
    for _, a, b in gen.next_epoch():
        b3.append(np.array(a, dtype=np.float32)), b2.append(np.array(b, dtype=np.float32)), sizes.append(len(a))
    rec["v_b3d"], rec["v_b2d"], rec["v_sizes"] = np.concatenate(b3), np.concatenate(b2), np.array(sizes, dtype=np.int32)
    vnet = EU.StubVideoPosenet(vw)
    for flip in ("", "_flip"):
        r = V.video_mode_evaluate(EU.video_args(), gen, vnet, torch.device("cpu"), flipaug=flip, get_pck_auc=True)
        rec["v_" + ("flip" if flip else "noflip")] = np.array(r, dtype=np.float64)

    for name, f in (("mpjpe", L.mpjpe), ("p_mpjpe", L.p_mpjpe), ("compute_PCK", L.compute_PCK),
                    ("compute_AUC", L.compute_AUC), ("evaluate", ME.evaluate), ("evaluate_posenet", ME.evaluate_posenet),
                    ("video_mode_evaluate", V.video_mode_evaluate),
                    ("video_mode_evaluate_posenet", V.video_mode_evaluate_posenet)):
        rec["sig_" + name] = sig(f)
    out = os.path.join(HERE, "pose_eval.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
