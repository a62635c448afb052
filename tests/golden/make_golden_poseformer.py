#!/usr/bin/env python3
"""Generate tests/golden/posenet_poseformer.npz and posenet_poseformer_f32.npz by RUNNING THE REFERENCE's PoseTransformer and
video_mode_train_posenet on the CPU (build container only: the reference is imported through tests/golden/_ref_import.py; one
thread).  Re-run with
    python tests/golden/make_golden_poseformer.py

The reference's module imports timm, which is not installed: empty stand-ins for timm.data, timm.models.helpers,
timm.models.layers and timm.models.registry are installed before the import (the class reads DropPath only, and only at a rate
above 0: every run here has rate 0, where the reference builds nn.Identity).  Weights and inputs are regenerated from seeds by both
sides (tests/poseformer_util.py) and are not stored; the seeded state gives the position embeddings (zero at initialisation) and the
LayerNorm affines random values.
posenet_poseformer.npz, the yardstick (the reference class converted with .double()):
  keys_<f> / shapes_<f> / dtypes_<f> / param_count_<f>   the reference's state_dict layout at its own configuration (16 joints, ratio 32,
                                                         depth 4, 8 heads), f = 9 and 27 frames
  init_<key>                                             torch.manual_seed, construction, .apply(init_weights) (poseformer_util.INIT)
  a<B>_f64_* (B = 7, 2; 3 frames, 5 joints, ratio 16,    out (training mode), loss, grad_<key>, eval_out as golden_util.compact records
              depth 2, 4 heads)                          (poseformer_util.COMPACT): every tensor up to 4 096 elements whole, i.e. all
                                                         but the weight gradients of the temporal blocks, which are samples + projections
  a27_f64_*  (27 frames, 16 joints, ratio 16, depth 1,   the same with fewer samples
              4 heads, B = 3)
  b_f64_*    (the reference's configuration at 9 frames, the same
              B = 6)
  c_final_<key>, c_losses, c_norms                       the reference's video_mode_train_posenet with its own class in fp64 (record
                                                         (a)'s configuration at 16 joints): 160 clips, batches 64, 64, 32, flip and
                                                         playback on, Adam lr 1e-3: the state after the 12 steps (compact records), the criterion's value
                                                         and clip_grad_norm_'s result per step.  fp64 because the k third of every qkv
                                                         bias has an identically zero gradient: in fp32 Adam walks on its rounding residue
posenet_poseformer_f32.npz, the class as it is (fp32): a<B>_f32_*, a27_f32_*, b_f32_* (same seeds)."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI        # noqa: E402
import golden_util as GU        # noqa: E402
import poseformer_util as FU    # noqa: E402
import posetrain_util as PU     # noqa: E402

torch.set_num_threads(1)


def install_timm_stubs():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()
            raise RuntimeError("the records are made at drop path 0: the stand-in DropPath must not be built")

    stub("timm")
    stub("timm.data", IMAGENET_DEFAULT_MEAN=0, IMAGENET_DEFAULT_STD=0)
    stub("timm.models")
    stub("timm.models.helpers", load_pretrained=None)
    stub("timm.models.layers", DropPath=DropPath, to_2tuple=None, trunc_normal_=None)
    stub("timm.models.registry", register_model=lambda f: f)


def build(Ref, cfg, dtype):
    m = Ref(**FU.kwargs(cfg))
    m.load_state_dict(FU.seeded_state(cfg), strict=True)
    return m.to(dtype)


def run(Ref, cfg, B, dtype):
    x, t = FU.inputs_of(cfg, B)
    return FU.run_record(build(Ref, cfg, dtype), x.to(dtype), t.to(dtype))


def main():
    RI.install_stubs()
    install_timm_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from models_baseline.poseformer.model_poseformer import PoseTransformer as Ref
    from models_baseline.mlp.linear_model import init_weights
    from models_Fk_GAN import video_mode_operate as V

    out, f32 = {}, {}
    for frames in FU.LAYOUTS:
        sd = Ref(**FU.kwargs(FU.reference_cfg(frames), 0)).state_dict()
        out["keys_%d" % frames] = np.array(list(sd.keys()))
        out["shapes_%d" % frames] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        out["dtypes_%d" % frames] = np.array([str(v.dtype) for v in sd.values()])
        out["param_count_%d" % frames] = np.array(sum(v.numel() for v in sd.values()))
    torch.manual_seed(FU.INIT["seed"])
    for k, v in Ref(**FU.kwargs(FU.INIT)).apply(init_weights).state_dict().items():
        out["init_" + k] = v.numpy().copy()

    def keep(rec, store, prefix, tag):
        for i, (k, v) in enumerate(rec):
            for part, a in GU.compact(v, i, **FU.COMPACT[tag]).items():
                store["%s%s__%s" % (prefix, k, part)] = a.numpy()
            store["%s%s__numel" % (prefix, k)] = np.array(v.numel())

    for tag, cfg, B in [("a", FU.SMALL, B) for B in FU.ROWS_A] + [("a27", FU.SMALL27, FU.ROWS_A27), ("b", FU.REF9, FU.ROWS_B)]:
        name = "a%d" % B if tag == "a" else tag
        r64, r32 = run(Ref, cfg, B, torch.float64), run(Ref, cfg, B, torch.float32)
        assert [k for k, _ in r64] == [k for k, _ in r32] == FU.record_names(cfg)
        keep(r64, out, name + "_f64_", tag)
        keep(r32, f32, name + "_f32_", tag)
        own = FU.errors_between(out, name + "_f64_", f32, name + "_f32_", FU.record_names(cfg))
        print("%s: fp32 vs fp64, worst tensor %.2e (%s)" % (name, max(own.values()), max(own, key=own.get)))

    # (c): the reference's video loop with its own class in fp64; the loop hands the model fp32 tensors, so the input and the
    # target are widened on the way in (the values are the fp32 ones)
    model = build(Ref, FU.LOOP, torch.float64)
    model.register_forward_pre_hook(lambda m, args: (args[0].double(),))
    batches = [(b3.double().numpy(), b2.double().numpy()) for b3, b2 in FU.train_batches()]
    clip, norms, losses = nn.utils.clip_grad_norm_, [], []

    class Crit(nn.Module):
        def forward(self, a, b):
            loss = nn.functional.mse_loss(a, b.to(a.dtype))
            losses.append(float(loss.item()))
            return loss

    def recording_clip(*a, **k):
        r = clip(*a, **k)
        norms.append(float(r))
        return r

    nn.utils.clip_grad_norm_ = recording_clip
    try:
        V.video_mode_train_posenet(model, PU.loader_of("video", batches), torch.optim.Adam(model.parameters(), lr=FU.TRAIN["lr"]),
                                   Crit(), torch.device("cpu"), PU.loop_args())
    finally:
        nn.utils.clip_grad_norm_ = clip
    for i, (k, v) in enumerate(model.state_dict().items()):
        for part, a in GU.compact(v, i, **FU.COMPACT["c"]).items():
            out["c_final_%s__%s" % (k, part)] = a.numpy()
    out["c_losses"], out["c_norms"] = np.array(losses), np.array(norms)
    print("loop:", len(norms), "steps, norms %.3f .. %.3f, loss %.4f -> %.4f" % (min(norms), max(norms), losses[0], losses[-1]))
    init = FU.seeded_state(FU.LOOP)
    print("k thirds moved at most %.2e" % max((FU.key_third(v.double() - init[k].double())).abs().max().item()
                                               for k, v in model.state_dict().items() if k.endswith("qkv.bias")))

    for name, rec in (("posenet_poseformer.npz", out), ("posenet_poseformer_f32.npz", f32)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
