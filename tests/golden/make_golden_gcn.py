#!/usr/bin/env python3
"""Generate tests/golden/posenet_gcn.npz and posenet_gcn_f32.npz by RUNNING THE REFERENCE's SemGCN and train_posenet on the CPU (build
container only: the reference is imported through tests/golden/_ref_import.py; one thread).  Re-run with
    python tests/golden/make_golden_gcn.py

The reference's graph_utils.py needs scipy and is not imported: the adjacency comes from tests/gcn_util.py (the 16-joint parents,
row-normalised as adj_mx_from_edges does it; SemGraphConv reads only its pattern, which is recorded).  Weights and inputs are
regenerated from seeds by both sides (tests/gcn_util.py) and are not stored; every e is drawn from N(1, 0.5^2), so no adjacency is
uniform.  Dropout is off everywhere.
posenet_gcn.npz, the yardstick (the reference class converted with .double(); its SemGraphConv keeps adj in fp32 and fails on the
scatter of a double e, so every instance's adj ATTRIBUTE is converted as well):
  keys_128_4 / shapes_128_4 / dtypes_128_4 / param_count   the reference's state_dict layout at hid 128, 4 blocks
  adj_mask, parents                                        the pattern (adj > 0) and the skeleton it comes from
  init_<key>                                               the reference's initial state under torch.manual_seed (gcn_util.INIT)
  a<B>_f64_* (B = 6, 37; hid 32, 2 blocks)                 whole tensors: out (training mode), loss, grad_<key>, buf_<key> (BatchNorm
                                                           buffers after the forward), eval_out (evaluation-mode output after it)
  b_f64_*  (hid 128, 4 blocks, B = 96)                     the same through golden_util.compact records
  c_final_<key>, c_losses, c_norms                         the reference's train_posenet with its own class (hid 32, 2 blocks) on
                                                           posenet_util.train_data(): batch 96 and a last batch of 40, flip on, Adam
                                                           lr 1e-3: the state after the 12 steps, the criterion's value and
                                                           clip_grad_norm_'s result per step
posenet_gcn_f32.npz, the class as it is (fp32): a<B>_f32_*, b_f32_* (same seeds)."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import _ref_import as RI     # noqa: E402
import gcn_util as CU        # noqa: E402
import golden_util as GU     # noqa: E402
import posenet_util as NU    # noqa: E402
import posetrain_util as PU  # noqa: E402

torch.set_num_threads(1)


def build(Ref, Conv, cfg, dtype=torch.float32):
    model = Ref(CU.adj_matrix(), cfg["hid"], num_layers=cfg["blocks"], p_dropout=None)
    model.load_state_dict(CU.seeded_state(cfg["hid"], cfg["blocks"], cfg["seed"]), strict=True)
    model = model.to(dtype)
    for mod in model.modules():
        if isinstance(mod, Conv):
            mod.adj = mod.adj.to(dtype)
    return model


def run(Ref, Conv, cfg, B, dtype):
    x, t = CU.inputs_of(cfg, B)
    return CU.run_record(build(Ref, Conv, cfg, dtype), x.to(dtype), t.to(dtype))


def main():
    RI.install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    os.chdir(RI.REF_ROOT)
    from models_baseline.gcn.sem_gcn import SemGCN as Ref
    from models_baseline.gcn.sem_graph_conv import SemGraphConv as Conv
    from function_aug import model_pos_train as MT

    out = {}
    ref = Ref(CU.adj_matrix(), 128, num_layers=4, p_dropout=0.25)
    sd = ref.state_dict()
    out["keys_128_4"] = np.array(list(sd.keys()))
    out["shapes_128_4"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    out["dtypes_128_4"] = np.array([str(v.dtype) for v in sd.values()])
    out["param_count"] = np.array(sum(p.numel() for p in ref.parameters()))
    out["adj_mask"] = (ref.gconv_output.adj > 0).numpy()
    out["parents"] = np.array(CU.PARENTS)
    assert np.array_equal(out["adj_mask"], CU.adj_mask())
    torch.manual_seed(CU.INIT["seed"])
    for k, v in Ref(CU.adj_matrix(), CU.INIT["hid"], num_layers=CU.INIT["blocks"], p_dropout=0.25).state_dict().items():
        out["init_" + k] = v.numpy().copy()

    f32 = {}
    dist = lambda a, r: (a.double() - r).abs().max().item() / max(r.abs().max().item(), 1e-300)
    for B in CU.ROWS_A:
        a64, a32 = run(Ref, Conv, CU.SMALL, B, torch.float64), run(Ref, Conv, CU.SMALL, B, torch.float32)
        for (k, v), (k32, v32) in zip(a64, a32):
            assert k == k32
            out["a%d_f64_%s" % (B, k)] = v.numpy()
            f32["a%d_f32_%s" % (B, k)] = v32.numpy()
        print("hid 32, B = %d: fp32 vs fp64, worst tensor %.2e" % (B, max(dist(v32, v) for (_, v), (_, v32) in zip(a64, a32)
                                                                           if v.dtype.is_floating_point)))

    r64, r32 = run(Ref, Conv, CU.WIDE, CU.ROWS_B, torch.float64), run(Ref, Conv, CU.WIDE, CU.ROWS_B, torch.float32)
    for i, ((k, v), (_, v32)) in enumerate(zip(r64, r32)):
        if v.dtype.is_floating_point:
            for part, a in GU.compact(v, i).items():
                out["b_f64_%s__%s" % (k, part)] = a.numpy()
            for part, a in GU.compact(v32, i).items():
                f32["b_f32_%s__%s" % (k, part)] = a.numpy()
        else:
            out["b_f64_" + k] = v.numpy()
            f32["b_f32_" + k] = v32.numpy()
    print("wide fp32 vs fp64, worst tensor: %.2e" % max(dist(v32, v) for (_, v), (_, v32) in zip(r64, r32) if v.dtype.is_floating_point))

    # (c): the reference's loop with its own class
    model = build(Ref, Conv, CU.SMALL)
    p3, p2 = NU.train_data()
    B = NU.TRAIN["batch"]
    batches = [(p3[i:i + B], p2[i:i + B]) for i in range(0, NU.TRAIN["n"], B)]
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
        MT.train_posenet(model, PU.loader_of("single", batches), torch.optim.Adam(model.parameters(), lr=NU.TRAIN["lr"]), Crit(),
                         torch.device("cpu"), PU.loop_args())
    finally:
        nn.utils.clip_grad_norm_ = clip
    for k, v in model.state_dict().items():
        out["c_final_" + k] = v.numpy().copy()
    out["c_losses"], out["c_norms"] = np.array(losses), np.array(norms)
    print("loop:", len(norms), "steps, norms %.3f .. %.3f, loss %.4f -> %.4f" % (min(norms), max(norms), losses[0], losses[-1]))

    for name, rec in (("posenet_gcn.npz", out), ("posenet_gcn_f32.npz", f32)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
