"""Throughput of the batched inverse-kinematics fit (dhaug_ik_fit), reported in the README, not gated.

    python tools/time_ik.py [--poses 65536] [--iters 12] [--rounds 5] [--cpu-poses 2048] [--cold] [--staged]

GPU: poses per second of ops.ik_fit on the trial's warm-start inputs (tests/ik_util.py: 5 degrees off per live slot), HIP events
around one call, median of `--rounds` rounds after one untimed call; the convergence share and the residual distribution of the
last round (by the kernel's own residual) are printed with it.  CPU, for scale: the fp64 restatement of tests/ik_util.py
(autograd Jacobian, batched Cholesky) on 16 threads at `--cpu-poses` poses.  --cold adds the share of 1 000 poses that converge
from the T-pose in 40 steps, and the tracking share on 128 sequences of 24 frames.  --staged times the coarse-to-fine fit
(ops.IK_COARSE_TO_FINE, 40 steps from the T-pose) against the single-stage fit with 40 steps on the same poses, the two taking
turns in one process, and counts what each leaves not converged on 1 000 poses (and skips the CPU part).  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-poses", type=int, default=2048)
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--staged", action="store_true")
    a = ap.parse_args()
    import dhaug_amd  # noqa: F401
    from dhaug_amd import ops
    import ik_util as K

    period = 4096                                             # distinct poses; the batch repeats them (the oracle's FK makes the targets)
    d = K.trial_fit_inputs(period)
    idx = torch.arange(a.poses) % period
    pose, init = d["pose"][idx].cuda(), d["init"][idx].cuda()
    fit = ops.ik_fit(pose, init, iters=a.iters)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fit = ops.ik_fit(pose, init, iters=a.iters)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    res = fit.residual[:period].double().cpu()
    q = torch.quantile(res, torch.tensor([0.5, 0.9, 0.99], dtype=torch.float64)).tolist()
    out = {"poses": a.poses, "iters": a.iters, "rounds": a.rounds, "gpu_ms_median": statistics.median(ms), "gpu_ms_all": ms,
           "gpu_poses_per_s": a.poses / (statistics.median(ms) * 1e-3), "warm_distinct_poses": period,
           "warm_not_converged": int((res > K.CONVERGED_M).sum()), "residual_median_m": q[0], "residual_p90_m": q[1],
           "residual_p99_m": q[2], "residual_max_m": res.max().item()}

    if a.staged:
        weights, steps = zip(*ops.IK_COARSE_TO_FINE)
        total = sum(steps)
        runs = {"single": lambda: ops.ik_fit(pose, None, iters=total), "staged": lambda: ops.ik_fit_staged(pose, weights, steps)}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        ms2 = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms2[k].append(e0.elapsed_time(e1))
        cold = d["pose"][:1000].cuda()
        out.update({"staged_steps": total, "staged_ms_median": statistics.median(ms2["staged"]), "staged_ms_all": ms2["staged"],
                    "single_ms_median": statistics.median(ms2["single"]), "single_ms_all": ms2["single"], "cold_poses": 1000,
                    "staged_not_converged": int((ops.ik_fit_staged(cold, weights, steps).residual > K.CONVERGED_M).sum()),
                    "single_not_converged": int((ops.ik_fit(cold, None, iters=total).residual > K.CONVERGED_M).sum())})
        print(json.dumps(out))
        return

    torch.set_num_threads(16)
    n = a.cpu_poses
    t0 = time.perf_counter()
    K.lm_fit(d["pose"][:n], d["init"][:n], iters=a.iters)
    dt = time.perf_counter() - t0
    out.update({"cpu_poses": n, "cpu_threads": torch.get_num_threads(), "cpu_s": dt, "cpu_poses_per_s": n / dt})

    if a.cold:
        cold = ops.ik_fit(d["pose"][:1000].cuda(), None, iters=40)
        out["cold_poses"] = 1000
        out["cold_not_converged"] = int((cold.residual > K.CONVERGED_M).sum())
        t = K.trial_track_inputs(128)
        tr = ops.ik_track(t["pose"].cuda(), t["offsets"], t["init"].cuda(), iters=8)
        out["track_frames"] = int(tr.residual.numel())
        out["track_not_converged"] = int((tr.residual > K.CONVERGED_M).sum())
        out["track_residual_max_m"] = tr.residual.max().item()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
