#!/usr/bin/env python3
"""Generate tests/golden/pose_eval_detail.npz by RUNNING THE REFERENCE's mpjpe_byjoint, weighted_mpjpe, n_mpjpe and
mean_velocity_error (utils/loss.py) on the CPU (build container only: the reference is imported through
tests/golden/_ref_import.py, with its root on sys.path and as working directory).  Re-run with
    python tests/golden/make_golden_eval_detail.py

Contents (data only; the case builders are tests/eval_util.py's):
  cases                              the case names: noisy, similarity (eval_util.metric_cases), millimetres, kilometres (the
                                     recipe of metric_cases' cases of these names on 128 poses)
  <case>_pred / _target              fp32 (128, 16, 3); the 4-D form of every record below is their reshape to (32, 4, 16, 3)
  w_j4 (32,4,16), w_p4 (32,4,1), w_b4 (32,1,1), w_j3 (128,16), w_p3 (128,1)      fp32 weights, negative ones included
  <case>_<record>_ref32 / _ref64     the reference's result on the fp32 inputs, and on the same values cast to fp64:
      bj3, bj4                       mpjpe_byjoint of the 3-D / 4-D form: (16,), (4, 16)
      wj4, wp4, wb4, wj3, wp3        weighted_mpjpe with the weights of that name
      n4                             n_mpjpe of the 4-D form
      v3, v4                         mean_velocity_error of the 3-D / 4-D form (numpy)
  sig_<function>                     the reference signatures
Every record is asserted finite."""
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

WEIGHTS = {"w_j4": (32, 4, 16), "w_p4": (32, 4, 1), "w_b4": (32, 1, 1), "w_j3": (128, 16), "w_p3": (128, 1)}


def cases():
    m = EU.metric_cases()
    out = {k: m[k] for k in ("noisy", "similarity")}
    rng = np.random.RandomState(2026)
    x = EU.skeleton(rng, 128)
    y = EU.grid(x + rng.randn(*x.shape).astype(np.float32) * 0.04)
    out["millimetres"] = ((y * 1000).astype(np.float32), (x * 1000).astype(np.float32))
    out["kilometres"] = ((y / 1000).astype(np.float32), (x / 1000).astype(np.float32))
    return out


def weights():
    rng = np.random.RandomState(11)
    out = {}
    for k, shape in WEIGHTS.items():
        w = rng.uniform(0.25, 2.0, size=shape)
        w[rng.uniform(size=shape) < 0.25] *= -1.0
        out[k] = EU.grid(w, 8)
    return out


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from utils import loss as L

    rec = {}
    W = weights()
    rec.update(W)
    names = []
    for name, (y, x) in cases().items():
        assert y.shape == (128, 16, 3) and y.dtype == np.float32 and x.dtype == np.float32
        names.append(name)
        rec[name + "_pred"], rec[name + "_target"] = y, x
        for tag, dt in (("ref32", np.float32), ("ref64", np.float64)):
            y3, x3 = y.astype(dt), x.astype(dt)
            y4, x4 = y3.reshape(32, 4, 16, 3), x3.reshape(32, 4, 16, 3)
            t = torch.from_numpy
            r = {"bj3": L.mpjpe_byjoint(t(y3), t(x3)).numpy(), "bj4": L.mpjpe_byjoint(t(y4), t(x4)).numpy(),
                 "n4": L.n_mpjpe(t(y4), t(x4)).numpy(),
                 "v3": np.asarray(L.mean_velocity_error(y3, x3)), "v4": np.asarray(L.mean_velocity_error(y4, x4))}
            for k, w in W.items():
                yy, xx = (y4, x4) if k.endswith("4") else (y3, x3)
                r[k.replace("_", "")] = L.weighted_mpjpe(t(yy), t(xx), t(w.astype(dt))).numpy()
            for k, v in r.items():
                assert v.dtype == dt and np.all(np.isfinite(v)), (name, k, tag)
                rec["%s_%s_%s" % (name, k, tag)] = v
    rec["cases"] = np.array(names)
    for f in (L.mpjpe_byjoint, L.weighted_mpjpe, L.n_mpjpe, L.mean_velocity_error):
        rec["sig_" + f.__name__] = np.array([str(inspect.signature(f))])
    out = os.path.join(HERE, "pose_eval_detail.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
