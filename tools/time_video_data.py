"""The device-resident video loader (models_Fk_GAN/video_mode_operate.py) on H36M-sized synthetic data: 600 camera-space
sequences of 150-400 frames (about H36M S1/5/6/7/8 at --downsample 10), roots at depth 3-6 m, real H36M intrinsics.

  (a) video_mode_dataloader_update: host clock around a synchronise (upload, bone swap, projection, record table)
  (b) a whole next_epoch() at R = 9, 27, 81 with B = 512: ms per batch (host clock, one synchronise at the end)
  (c) 20 video GAN iterations (B = 512, R = 9, DenseDim 1000, hipGraphs as bench.py runs them) fed by the loader, against the
      same 20 batches staged on the device beforehand; the two alternate, --reps times.  The loader's epoch start (host
      shuffle of the whole pair table + its upload, once per epoch of ~315 batches) is outside these 20 iterations: (b)
      reports it.

    python tools/time_video_data.py [--part abc] [--reps 5]
The kernel's own time: the same script under `rocprofv3 --kernel-trace --stats -- python tools/time_video_data.py --part b`."""
import argparse
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import dhaug_amd  # noqa: F401
from dhaug_amd.models_Fk_GAN import video_mode_operate as VO
from video_data_util import synth_sequences


def ms(t0):
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def data_dict(seed=0):
    lengths = np.random.RandomState(seed).randint(150, 401, 600)
    poses, cams = synth_sequences(lengths, seed)
    return dict(poses_train=poses, poses_train_2d=[np.zeros((len(p), 16, 2), np.float32) for p in poses],
                actions_train=["a"] * len(poses), cams_train=cams)


def update(data, B, arch):
    VO.video_mode_dataloader_update(argparse.Namespace(batch_size=B, architecture=arch), data, torch.device("cuda"))
    return data["target_GAN_loader"]


def part_a(data):
    frames = sum(len(p) for p in data["poses_train"])
    ts = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        update(data, 512, "3,3")
        ts.append(ms(t0))
    print("(a) video_mode_dataloader_update, %d sequences, %d frames: %s ms (the first one includes warm-up)"
          % (len(data["poses_train"]), frames, " ".join("%.2f" % t for t in ts)))


def part_b(data):
    for arch in ("3,3", "3,3,3", "3,3,3,3"):
        g = update(data, 512, arch)
        R = g.frames
        for b in g.next_epoch():            # warm-up epoch (allocator, code objects)
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = g.next_epoch()
        next(it)
        t_start = ms(t0)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for b in g.next_epoch():
                n += 1
            ts.append(ms(t0) / n)
        mb = 512 * R * 80 * 4 / 1e6
        print("(b) R = %2d, B = 512: %d batches, %.2f MB each: %s ms per batch; epoch start (shuffle of %d pairs, record "
              "upload, first batch) %.2f ms" % (R, n, mb, " ".join("%.4f" % t for t in ts), len(g.pairs), t_start))


def part_c(data, reps):
    from dhaug_amd.common.camera import camera_params9
    from dhaug_amd.common.h36m_dataset import h36m_cameras_extrinsic_params, h36m_cameras_intrinsic_params
    from dhaug_amd.function_aug.config import synth_args
    from dhaug_amd.graphs import GraphedGanIteration
    from dhaug_amd.models_Fk_GAN import model_fk_gan_train as T, video_GAN_fun as V
    from dhaug_amd.models_Fk_GAN.forward_kinematics_DH_model import Forward_Kinematics_DH_Model
    B, D, R, N = 512, 1000, 9, 20
    ext = h36m_cameras_extrinsic_params["S1"][0]
    camera = ([float(v) for v in ext["orientation"]], [float(v) / 1000.0 for v in ext["translation"]],
              camera_params9(h36m_cameras_intrinsic_params[0]))
    args = synth_args(B, D, single_or_multi_train_mode="multi", architecture="3,3", video_Dis_DenseDim_3D=D,
                      video_Dis_DenseDim_2D=D, single_dis_warmup_epoch=0)
    models = T.video_mode_my_get_poseFk_model(args, None, Forward_Kinematics_DH_Model(args, ["S1"], None), R)
    g = update(data, B, "3,3")
    staged = []
    for b in g.next_epoch():
        staged.append(b)
        if len(staged) == N:
            break
    cam0, x30, x20 = staged[0]
    models["model_G"].GAN_generator_get_bone_length(x30.reshape(-1, 16, 3))
    gv = GraphedGanIteration(V.video_gan_iteration, args, models, ["S1"], argparse.Namespace(epoch=10, train_iter_num=0))
    for i in range(10):
        gv(x30, cam0, x20, i % 5 == 4, camera)
    torch.cuda.synchronize()

    def fed(source):
        source = iter(source)
        first = next(source)                # (the loader's epoch start -- host shuffle + record upload -- is timed in (b))
        source = itertools.chain([first], source)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (cam, x3, x2) in zip(range(N), source):
            gv(x3, cam, x2, i % 5 == 4, camera)
        return ms(t0) / N

    res = {"loader": [], "staged": []}
    for _ in range(reps):
        res["loader"].append(fed(g.next_epoch()))
        res["staged"].append(fed(iter(staged)))
    for k, v in res.items():
        print("(c) %d iterations fed by %-6s: %s ms per iteration (median %.3f)" % (N, k, " ".join("%.3f" % t for t in v),
                                                                                np.median(v)))
    print("(c) loader / staged (medians): %.4f" % (np.median(res["loader"]) / np.median(res["staged"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abc")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    data = data_dict()
    if "a" in a.part:
        part_a(data)
    if "b" in a.part:
        part_b(data)
    if "c" in a.part:
        part_c(data, a.reps)


if __name__ == "__main__":
    main()
