#!/usr/bin/env python3
"""Generate tests/golden/posenet_mlp.npz and posenet_mlp_f32.npz by RUNNING THE REFERENCE's LinearModel (models_baseline/mlp) and
train_posenet on the CPU (build container only: the reference is imported through tests/golden/_ref_import.py; one thread).
Re-run with
    python tests/golden/make_golden_linear_model.py

Weights and inputs are regenerated from seeds by both sides (tests/linear_model_util.py, tests/posenet_util.py) and are not stored.
Dropout is 0 everywhere.  posenet_mlp.npz, the yardstick (the reference class converted with .double()):
  keys_<C>_<stages> / shapes_ / dtypes_         the reference's state_dict layout at (1 024, 2) and (1 024, 4)
  init_<key>                                    the state after torch.manual_seed + construction + apply(init_weights), C = 64
  a<M>_f64_* (M = 96, 40; C = 64, stages 2)     whole tensors: out (training mode), loss, grad_<key>, buf_<key> (BatchNorm buffers
                                                after the forward), eval_out (evaluation-mode output after it)
  b_f64_*  (C = 1 024, stages 2, M = 96)        the same through golden_util.compact records (<name>__full | __sample, __proj)
  c_final_<key>, c_losses, c_norms              the reference's train_posenet with its own class (C = 64, stages 2) IN FP64 (a
                                                .double() model and double pairs; the loop casts nothing): 520 pairs, batch 96 and
                                                a last batch of 40, flip on, Adam lr 1e-3: the state after the 12 steps, the
                                                criterion's value and clip_grad_norm_'s result per step
posenet_mlp_f32.npz, the class as it is (fp32): a<M>_f32_*, b_f32_* as above, same seeds.

The bias of a Linear in front of a training-mode BatchNorm has a zero gradient in exact arithmetic, and the package treats it as a
constant.  The tests rely on the fp64 reference behaving so, which is asserted here before anything is written: in (a) and (b)
every such gradient is <= 1e-12 x the largest weight-gradient element, and in (c) every such bias moves <= 1e-9."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI         # noqa: E402
import golden_util as GU         # noqa: E402
import linear_model_util as LU   # noqa: E402
import posetrain_util as PU      # noqa: E402

torch.set_num_threads(1)


def build(cls, cfg, dtype):
    model = cls(32, 45, linear_size=cfg["C"], num_stage=cfg["stages"], p_dropout=0.0)
    model.load_state_dict(LU.seeded_state(cfg["C"], cfg["stages"], cfg["seed"]), strict=True)
    return model.to(dtype)


def run(cls, cfg, M, dtype):
    """training-mode forward + MSE backward, then the evaluation-mode forward, of the reference class"""
    model = build(cls, cfg, dtype)
    x, t = LU.make_inputs(M, cfg["seed"] + 100 + M)
    x, t = x.to(dtype), t.to(dtype)
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
    return rec


def check_bias_gradients(rec, stages, what):
    wmax = max(v.abs().max().item() for k, v in rec.items() if k.startswith("grad_") and k.endswith(".weight") and "batch_norm" not in k)
    worst = max(rec["grad_" + k].abs().max().item() for k in LU.pre_bn_biases(stages))
    print("%s: largest pre-BN bias gradient %.2e, largest weight-gradient element %.2e" % (what, worst, wmax))
    assert worst <= 1e-12 * wmax, (what, worst, wmax)


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from models_baseline.mlp.linear_model import LinearModel as Ref, init_weights
    from function_aug import model_pos_train as MT

    out = {}
    for C, stages in LU.LAYOUTS:
        sd = Ref(32, 45, linear_size=C, num_stage=stages, p_dropout=0.25).state_dict()
        tag = "%d_%d" % (C, stages)
        out["keys_" + tag] = np.array(list(sd.keys()))
        out["shapes_" + tag] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        out["dtypes_" + tag] = np.array([str(v.dtype) for v in sd.values()])
    torch.manual_seed(LU.INIT["seed"])
    init = Ref(32, 45, linear_size=LU.INIT["C"], num_stage=LU.INIT["stages"]).apply(init_weights)
    for k, v in init.state_dict().items():
        out["init_" + k] = v.numpy().copy()

    f32 = {}
    dist = lambda a, ref: (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)
    for M in LU.ROWS_A:
        a64, a32 = run(Ref, LU.SMALL, M, torch.float64), run(Ref, LU.SMALL, M, torch.float32)
        check_bias_gradients(a64, LU.SMALL["stages"], "a%d" % M)
        for k, v in a64.items():
            out["a%d_f64_%s" % (M, k)] = v.numpy()
            f32["a%d_f32_%s" % (M, k)] = a32[k].numpy()
        print("C = 64, M = %d: fp32 vs fp64, worst tensor %.2e" % (M, max(
            dist(a32[k], v) for k, v in a64.items() if v.dtype.is_floating_point and k[5:] not in LU.pre_bn_biases(2))))

    r64, r32 = run(Ref, LU.WIDE, LU.ROWS_B, torch.float64), run(Ref, LU.WIDE, LU.ROWS_B, torch.float32)
    check_bias_gradients(r64, LU.WIDE["stages"], "b")
    for i, (k, v) in enumerate(r64.items()):
        if v.dtype.is_floating_point:
            for part, a in GU.compact(v, i).items():
                out["b_f64_%s__%s" % (k, part)] = a.numpy()
            for part, a in GU.compact(r32[k], i).items():
                f32["b_f32_%s__%s" % (k, part)] = a.numpy()
        else:
            out["b_f64_" + k] = v.numpy()
            f32["b_f32_" + k] = r32[k].numpy()

    # (c): the reference's loop with its own class, in fp64
    cfg = LU.SMALL
    model = build(Ref, cfg, torch.float64)
    first = {k: model.state_dict()[k].clone() for k in LU.pre_bn_biases(cfg["stages"])}
    p3, p2 = LU.train_data()
    p3, p2 = p3.double(), p2.double()
    B = LU.TRAIN["batch"]
    batches = [(p3[i:i + B], p2[i:i + B]) for i in range(0, LU.TRAIN["n"], B)]
    clip, norms, losses = nn.utils.clip_grad_norm_, [], []

    class Crit(nn.Module):
        def forward(self, a, b):
            assert a.dtype == b.dtype == torch.float64
            loss = nn.functional.mse_loss(a, b)
            losses.append(float(loss.item()))
            return loss

    def recording_clip(*a, **k):
        r = clip(*a, **k)
        norms.append(float(r))
        return r

    nn.utils.clip_grad_norm_ = recording_clip
    try:
        MT.train_posenet(model, PU.loader_of("single", batches), torch.optim.Adam(model.parameters(), lr=LU.TRAIN["lr"]), Crit(),
                         torch.device("cpu"), PU.loop_args())
    finally:
        nn.utils.clip_grad_norm_ = clip
    moved = max((model.state_dict()[k] - v).abs().max().item() for k, v in first.items())
    print("loop:", len(norms), "steps, norms %.3f .. %.3f, loss %.4f -> %.4f; pre-BN biases moved %.2e"
          % (min(norms), max(norms), losses[0], losses[-1], moved))
    assert len(norms) == 12 and moved <= 1e-9, moved
    for k, v in model.state_dict().items():
        assert v.dtype in (torch.float64, torch.int64)
        out["c_final_" + k] = v.numpy().copy()
    out["c_losses"], out["c_norms"] = np.array(losses), np.array(norms)

    for name, rec in (("posenet_mlp.npz", out), ("posenet_mlp_f32.npz", f32)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
