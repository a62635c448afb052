"""development: the launch trace of the explicit critic and generator steps (critic_step.py, gen_step.py) -- the counterpart of
tools/same_isa.py for the Python schedule.  A change that only reorganises the schedule leaves every line of the output as it was.

    python tools/step_trace.py OUT.jsonl            one JSON line per case
    python tools/step_trace.py --compare A B        exit status 1 unless every case of A and B is equal

Every C-ABI call of a case is recorded through _lib.call (as tools/count_calls.py counts them): its name and its arguments by the
types of _lib.SIGNATURES -- a pointer as 0, as "p", or as "=k" where it equals the k-th pointer of the same call (in-place aliasing,
whatever the allocator hands out); the stream (last argument) as the index of its handle's first appearance in the case; everything
else by value; the elements of a descriptor array field by field, by the same rules.  After the step: sha256 (and, to size a difference, the norms) of the
scalars it returned and of every parameter of the stepped network.  It reaches the steps through critic_step.critic_step, gen_step.generator_step
and the modules' switches alone, so one copy of this file runs against an older tree as well: run it on both, then --compare."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def compare(a, b):
    A, B = ([json.loads(l) for l in open(p)] for p in (a, b))
    print("%d / %d cases, %d / %d calls" % (len(A), len(B), sum(len(x["calls"]) for x in A), sum(len(y["calls"]) for y in B)))
    bad = len(A) != len(B)
    for x, y in zip(A, B):
        if x["case"] != y["case"] or x["calls"] != y["calls"]:
            i = next((i for i, (c, d) in enumerate(zip(x["calls"], y["calls"])) if c != d), min(len(x["calls"]), len(y["calls"])))
            print("CALLS DIFFER", x["case"], "| call", i, x["calls"][i:i + 1], y["calls"][i:i + 1])
            bad = True
        elif x["sha256"] != y["sha256"]:
            # (same launches, other bits: by how much -- the order of fp32 atomic additions moves a norm in its last digits)
            rel = max(abs(p - q) / max(abs(p), 1e-30) for p, q in zip(x["norms"], y["norms"]))
            print("BITS DIFFER  %-60s max relative difference of a tensor's norm %.1e" % (x["case"], rel))
            bad = True
    print("different" if bad else "equal")
    sys.exit(1 if bad else 0)


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    compare(sys.argv[2], sys.argv[3])

import torch
import dhaug_amd
from dhaug_amd import _lib, critic_step as CS, gen_step as GS, ops
from dhaug_amd.common.camera import camera_params9
from dhaug_amd.common.h36m_dataset import h36m_cameras_extrinsic_params, h36m_cameras_intrinsic_params
from dhaug_amd.models_Fk_GAN import Fk_discriminator as dis, forward_kinematics_DH_model as fkm, model_fk_gan_train as train
import golden_util as GU
from test_gpu_models import make_args

STRUCTS = (_lib.GemmDesc, _lib.TnLayer, _lib.Block2, _lib.TopDesc, _lib.MlpUnit)
calls, streams = [], []
orig = _lib.call


def _ptr(v, seen):
    v = getattr(v, "value", v) or 0
    if v == 0:
        return 0
    seen.append(v)
    k = seen.index(v)
    return "p" if k == len(seen) - 1 else "=%d" % k


def _elements(v):
    if isinstance(v, ctypes.Array):
        return list(v)
    return [getattr(v, "_obj", v)]                   # (ctypes.byref(d))


def call(name, *args):
    sig, seen, rec = _lib.SIGNATURES[name], [], [name]
    for i, (t, v) in enumerate(zip(sig, args)):
        if i == len(sig) - 1:
            h = getattr(v, "value", v) or 0
            if h not in streams:
                streams.append(h)
            rec.append("s%d" % streams.index(h))
        elif t is ctypes.c_void_p:
            rec.append(_ptr(v, seen))
        elif isinstance(v, (ctypes.Array, ctypes.Structure)) or hasattr(v, "_obj"):
            for e in _elements(v):
                if isinstance(e, STRUCTS):
                    rec.append([_ptr(getattr(e, f), seen) if ft is ctypes.c_void_p else getattr(e, f) for f, ft in e._fields_])
                else:                                # (an array of pointers / numbers: dhaug_weighted_means)
                    rec.append(_ptr(e, seen) if v._type_ is ctypes.c_void_p else e)
        else:
            rec.append(v)
    calls.append(rec)
    return orig(name, *args)


_lib.call = call


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def case(out, name, fn, nets):
    """fn() -> the step's scalars; nets: the networks it steps"""
    CS._SEED_CACHE.clear()
    del calls[:], streams[:]
    r = fn()
    torch.cuda.synchronize()
    r = [r] if torch.is_tensor(r) else list(r)
    r += [p for n in nets for p in n.parameters()]
    out.write(json.dumps(dict(case=name, calls=calls, sha256=sha(r), norms=[t.detach().double().norm().item() for t in r])) + "\n")
    print("%-60s %4d calls" % (name, len(calls)), flush=True)


def critic(tag, D, B, prec, R=9):
    """(step, [net]) of one critic step: fresh seeded weights, batch and interpolation coefficients"""
    torch.manual_seed(11)
    gen = torch.Generator().manual_seed(5)
    if tag in ("d3", "d2"):
        args = make_args(batch_size=B, Dis_DenseDim_3D=D, Dis_DenseDim_2D=D)
        net = dis.Fk_3D_Discriminator("cuda", args) if tag == "d3" else dis.Fk_2D_Discriminator(args, 16)
        w = 3 if tag == "d3" else 2
        real = torch.randn(B, 16, w, generator=gen) * 0.3
        real = real - real[:, :1] if tag == "d3" else real
        fake = real + 0.05 * torch.randn(B, 16, w, generator=gen)
        fake = fake - fake[:, :1] if tag == "d3" else fake
        alpha = torch.rand(B, 1, generator=gen)
        rows = B
    else:
        args = make_args(batch_size=B, single_or_multi_train_mode="multi", architecture="3,3", video_Dis_DenseDim_3D=D, video_Dis_DenseDim_2D=D)
        cls = dis.Video_motion_Fk_3D_Discriminator if tag == "m3" else dis.Video_motion_Fk_2D_Discriminator
        net = cls("cuda", args, R)
        w = 48 if tag == "m3" else 32
        real = torch.randn(B, R, w, generator=gen) * 0.3
        fake = real + 0.05 * torch.randn(B, R, w, generator=gen)
        rows = B if tag == "m3" else B * R
        alpha = torch.rand(rows, 1, generator=gen)
    net.precision = prec
    net = net.cuda()
    opt = train.FusedAdam(net.parameters(), lr=1e-4, betas=(0.5, 0.9))
    real, fake, alpha = (t.reshape(rows, -1).cuda() for t in (real, fake, alpha))
    assert CS.supported(net, opt, real, fake, rows)
    return (lambda: CS.critic_step(net, opt, real, fake, alpha, 10.0)), [net]


def generator(B, D, R, prec, flip):
    torch.manual_seed(13)
    video = R > 1
    args = make_args(batch_size=B, Gen_DenseDim=D, Dis_DenseDim_3D=D, Dis_DenseDim_2D=D, video_Dis_DenseDim_3D=D, video_Dis_DenseDim_2D=D,
                     **(dict(single_or_multi_train_mode="multi", architecture="3,3", GAN_3d_motion_loss_weight=0.7,
                             GAN_2d_motion_loss_weight=0.4) if video else {}))
    fk = fkm.Forward_Kinematics_DH_Model(args, ["S1"], None)
    d = train.video_mode_my_get_poseFk_model(args, None, fk, R) if video else train.my_get_poseFk_model(args, None, fk)
    keys = ["model_G", "model_d3d", "model_d2d"] + (["model_motion_d3d", "model_motion_d2d"] if video else [])
    for k in keys:
        d[k].precision = prec
    d["model_G"].GAN_generator_get_bone_length(GU.synth_pose16(B * R, seed=4).cuda())
    ext = h36m_cameras_extrinsic_params["S1"][1]
    cam = ([float(v) for v in ext["orientation"]], [float(v) / 1000.0 for v in ext["translation"]], camera_params9(h36m_cameras_intrinsic_params[1]))
    noise = torch.randn(B, 128, generator=torch.Generator().manual_seed(9)).cuda()
    scaler = (torch.randint(-200, 200, (B, 8), generator=torch.Generator().manual_seed(10)) / 1000.0).cuda()
    critics, weights = tuple(d[k] for k in keys[1:]), (1.0, 0.2, 0.7, 0.4)[:len(keys) - 1]
    assert GS.supported(d["model_G"], d["optimizer_G"], critics)
    return (lambda: GS.generator_step(args, d["model_G"], d["optimizer_G"], critics, weights, cam, flip, noise, scaler, frames=R,
                                      playback=video)), [d["model_G"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    out = open(ap.parse_args().out, "w")
    run = lambda name, made: case(out, name, *made)
    for tag in ("d2", "d3"):
        for D, B in ((256, 1024), (256, 1000), (32, 96)):
            run("critic %s D%d B%d bf16" % (tag, D, B), critic(tag, D, B, "bf16"))
        for prec in ("bf16x6", "bf16x3", "f16x3"):
            for D, B in ((256, 1024), (32, 96)):
                run("critic %s D%d B%d %s" % (tag, D, B, prec), critic(tag, D, B, prec))
    for tag in ("m3", "m2"):
        for B in (128, 512):
            run("critic %s D1000 B%d bf16" % (tag, B), critic(tag, 1000, B, "bf16"))
        run("critic %s D32 B16 bf16x6" % tag, critic(tag, 32, 16, "bf16x6"))
    for flip in (False, True):
        for prec in ("bf16", "bf16x6"):
            run("generator D256 B1024 R1 %s flip=%d" % (prec, flip), generator(1024, 256, 1, prec, flip))
        run("generator D1000 B64 R9 bf16 flip=%d" % flip, generator(64, 1000, 9, "bf16", flip))
    # each switch off, one at a time, on the D = 256, B = 1024 steps of the arithmetic it concerns
    both = ("bf16", "bf16x6")
    switches = [(CS, "TN_SPLIT", ("bf16",)), (CS, "PLANES", ("bf16x6",)), (CS, "PLANES_OUT", ("bf16x6",)), (CS, "SEED_CASTS", ("bf16",)),
                (CS, "SKIP_XHAT_SAVES", ("bf16",)), (CS, "FUSED_STEP_FORWARD", ("bf16",)), (CS, "D3_PENALTY_FUSED", ("bf16",)),
                (ops, "BLOCK2", ("bf16",)), (ops, "TOP_FUSED", ("bf16",)), (ops, "TN256", both)]
    for mod, sw, precs in switches:
        assert getattr(mod, sw) is True, sw
        setattr(mod, sw, False)
        for prec in precs:
            for tag in ("d2", "d3"):
                run("%s=0 critic %s D256 B1024 %s" % (sw, tag, prec), critic(tag, 256, 1024, prec))
            run("%s=0 generator D256 B1024 R1 %s flip=1" % (sw, prec), generator(1024, 256, 1, prec, True))
        setattr(mod, sw, True)
    CS.NT_GROUP = False
    run("NT_GROUP=0 critic m3 D1000 B512 bf16", critic("m3", 1000, 512, "bf16"))
    CS.NT_GROUP = True
    out.close()


main()
