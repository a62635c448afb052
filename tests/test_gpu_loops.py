"""GPU parity of the epoch loops against golden vectors captured from the REFERENCE's
own GAN_solutions_FK_generator / video_mode_GAN_solutions_FK_generator runs with recorded random draws
(tests/golden/make_golden_loops.py), in the fp32-grade arithmetic ('bf16x6').

What is compared, per loop: the generated pairs of every iteration (pos_3d_cam / 2D -- the product of the epoch), the
D_real / D_fake / Wasserstein_D series of every critic step in the reference's logging order, the generator's gradients at
the G step (flip-averaged loss; video: four adversarial terms incl. the (-1, R, 32) view of quirk q6) and every network's
weights after the five iterations.  Adam's first steps are lr * g / (|g| + eps): elements whose gradient is ~0 are
ill-conditioned, hence a quantile bound next to the hard bound of (steps * lr)."""
import argparse

import pytest
import torch

import golden_util as GU
import loop_util as LU

pytestmark = pytest.mark.gpu


class Writer:
    def __init__(self):
        self.s = {}

    def add_scalar(self, name, value, step=None):
        self.s.setdefault(name.split("/", 1)[1], []).append(float(value))


class Summary:
    def __init__(self, epoch=0):
        self.epoch, self.train_iter_num, self.train_discrim_iter_num = epoch, 0, 0


def maxabs(a, b):
    return (a.detach().double().cpu() - torch.as_tensor(b).double()).abs().max().item()


def weights_close(net, g, prefix, steps, lr=1e-4):
    worst = 0.0
    for k, p in net.named_parameters():
        ref = g[prefix + k].double()
        e = (p.detach().double().cpu() - ref).abs().reshape(-1)
        worst = max(worst, e.max().item())
        assert e.max().item() <= 1.05 * steps * lr, (prefix, k, e.max().item())
        if e.numel() >= 64:
            assert torch.quantile(e, 0.98).item() <= 2e-5, (prefix, k, torch.quantile(e, 0.98).item())
    return worst


def pairs_close(p3, p2, g):
    """generated pairs: 1e-5 of the coordinate scale (camera-space metres up to ~6, projections up to ~4 after the clamp)"""
    for got, ref in ((torch.cat(p3), g["buf_p3"]), (torch.cat(p2), g["buf_p2"])):
        assert maxabs(got, ref) <= 1e-5 * max(1.0, ref.abs().max().item()), (maxabs(got, ref), ref.abs().max().item())


def scalars_close(w, g, tol):
    ref = LU.scalar_series(g)
    assert set(ref) == set(w.s), (sorted(ref), sorted(w.s))
    for name, r in ref.items():
        got = torch.tensor(w.s[name], dtype=torch.float64)
        assert got.shape == r.shape, name
        assert maxabs(got, r) <= tol * max(1.0, r.abs().max().item()), (name, maxabs(got, r))


def grads_close(G, g, rel):
    for k, p in G.named_parameters():
        ref = g["gstep_grad__" + k]
        assert maxabs(p.grad, ref) <= 1e-7 + rel * ref.abs().max().item(), (k, maxabs(p.grad, ref), ref.abs().max().item())


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dhaug_amd
    dhaug_amd._lib.lib()
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model, model_fk_gan_train, video_GAN_fun
    return argparse.Namespace(fkm=forward_kinematics_DH_model, train=model_fk_gan_train, video=video_GAN_fun)


def _args(**over):
    from test_gpu_models import make_args
    return make_args(**over)


def test_single_frame_loop_vs_reference(M, golden):
    g = golden("gan_loop_D32")
    iters, B = g["real3d"].shape[0], g["real3d"].shape[1]
    args = _args(batch_size=B, flip_GAN_model_input=True)
    fk = M.fkm.Forward_Kinematics_DH_Model(args, ["S1", "S5"], None)
    d = M.train.my_get_poseFk_model(args, None, fk)
    for key, sd in zip(("model_G", "model_d3d", "model_d2d"), LU.single_state_dicts(g)):
        d[key].load_state_dict(sd)
        d[key].precision = "bf16x6"
    w, s = Writer(), Summary()
    p3, p2 = [], []
    for i in range(iters):
        last = i == iters - 1
        draws = M.train.Draws(noise=[g["noise"][i]] + ([g["noise"][iters]] if last else []),
                              scaler=[g["scaler"][i]] + ([g["scaler"][iters]] if last else []),
                              alpha=[g["alpha"][4 * i + j] for j in range(4)])
        cam = (g["cam_quat"][i].tolist(), g["cam_trans"][i].tolist(), g["buf_cam"][i * B].tolist())
        if last:                                      # critic weights as the G step sees them
            pass
        r = M.train.gan_iteration(args, d, g["real3d"][i], g["cam_param"], g["real2d"][i], ["S1", "S5"], s, w,
                                  do_g_step=last, camera=cam, draws=draws)
        assert not any(draws.q.values()), "recorded draws left over"
        p3.append(r["pos_3d_cam"]); p2.append(r["pos_2d"])
        s.train_iter_num += 1
    pairs_close(p3, p2, g)
    scalars_close(w, g, 2e-4)
    grads_close(d["model_G"], g, 2e-3)
    assert r["G_cost"] is not None and torch.isfinite(r["G_cost"]).item()
    worst = [weights_close(d[k], g, p, n) for k, p, n in (("model_d3d", "final_d3__", 10), ("model_d2d", "final_d2__", 10),
                                                           ("model_G", "final_G__", 1))]
    print("single-frame loop: worst weight error D3 %.2e D2 %.2e G %.2e" % tuple(worst))


def _run_single_loop(M, g, D, precision):
    iters, B = g["real3d"].shape[0], g["real3d"].shape[1]
    args = _args(batch_size=B, flip_GAN_model_input=True, Gen_DenseDim=D, Dis_DenseDim_3D=D, Dis_DenseDim_2D=D)
    fk = M.fkm.Forward_Kinematics_DH_Model(args, ["S1", "S5"], None)
    d = M.train.my_get_poseFk_model(args, None, fk)
    for key, sd in zip(("model_G", "model_d3d", "model_d2d"), LU.single_state_dicts(g, D)):
        d[key].load_state_dict(sd)
        d[key].precision = precision
    w, s = Writer(), Summary()
    p3, p2 = [], []
    for i in range(iters):
        last = i == iters - 1
        draws = M.train.Draws(noise=[g["noise"][i]] + ([g["noise"][iters]] if last else []),
                              scaler=[g["scaler"][i]] + ([g["scaler"][iters]] if last else []),
                              alpha=[g["alpha"][4 * i + j] for j in range(4)])
        cam = (g["cam_quat"][i].tolist(), g["cam_trans"][i].tolist(), g["buf_cam"][i * B].tolist())
        r = M.train.gan_iteration(args, d, g["real3d"][i], g["cam_param"], g["real2d"][i], ["S1", "S5"], s, w,
                                  do_g_step=last, camera=cam, draws=draws)
        assert not any(draws.q.values()), "recorded draws left over"
        p3.append(r["pos_3d_cam"]); p2.append(r["pos_2d"])
        s.train_iter_num += 1
    return d, w, p3, p2, r


@pytest.mark.parametrize("precision", ["bf16x6", "bf16"])
@pytest.mark.parametrize("D", [256, 1000])
def test_single_frame_loop_vs_reference_at_dense_dim_256(M, golden, precision, D, monkeypatch):
    """(D = 1000: the same loop at the reference's DEFAULT width, R/function_aug/config.py:101-109 -- gan_loop_D1000, B = 128: the frame
    critics' twenty steps and the G step through the video path's DenseDim-1000 training kernels: the 256 x 256-tile ping-pong NT
    kernel (DHAUG_GEMM_WIDE_MIN_TILES=1 lets the test's 384 rows reach it), the wide grouped weight-gradient contractions, adam_nt,
    the explicit G step at that width.)
    The reference's own five-iteration loop at the width of its README command and of the benchmark (gan_loop_D256).  At
    DenseDim 256 the iteration runs the kernels the timed training step runs -- the fused forward-with-save programs, the
    two-layer block kernel, the sign-bit masks, the grouped weight gradients, the explicit G step -- which the DenseDim-32
    loop never enters.
      bf16x6 (fp32-grade, layer by layer): pairs, scalars, G-step gradients and all weights at the DenseDim-32 tolerances;
      bf16 (the TIMED arithmetic): the pairs of the first iterations are the bf16 generator's (no golden tolerance), the
      scalars of all twenty critic steps within 5e-2, the G-step gradients and the weight changes by direction and size."""
    g = golden("gan_loop_D%d" % D)
    if D == 1000:
        monkeypatch.setenv("DHAUG_GEMM_WIDE_MIN_TILES", "1")
    d, w, p3, p2, r = _run_single_loop(M, g, D, precision)
    ref = LU.scalar_series(g)
    assert set(ref) == set(w.s)
    init = dict(zip(("model_G", "model_d3d", "model_d2d"), LU.single_state_dicts(g, D)))
    if precision == "bf16x6":
        # pairs: the generator's 256-wide trunk in six bf16 terms per product is ~1e-6 in the head; the root is 10 tanh(head) and
        # the projection divides by the camera depth, so the pairs are held to 1e-4 m / 3e-4 (measured: see the print)
        e3, e2 = maxabs(torch.cat(p3), g["buf_p3"]), maxabs(torch.cat(p2), g["buf_p2"])
        print("bf16x6 loop at D = %d: pairs differ by %.2e m (3D) / %.2e (2D)" % (D, e3, e2))
        # (D = 1000: four times the contraction length -- measured 1.3e-5 m / 3.0e-4; the 2D figure is one pose next to the camera plane)
        assert e3 <= 1e-4 and e2 <= (3e-4 if D == 256 else 6e-4), (e3, e2)
        # (D = 1000: the tenth critic step's D_real differs by 2.7e-4 -- nine sign-like Adam steps of 12 M parameters behind it)
        scalars_close(w, g, 2e-4 if D == 256 else 5e-4)
        worst = 0.0
        for i, (k, p) in enumerate(d["model_G"].named_parameters()):
            rec = LU.compact_record(g, "gstep_grad__", k)
            kk = "full" if "full" in rec else "sample"
            got = GU.compact(p.grad.detach().float().cpu(), 100 + i)
            worst = max(worst, (got[kk].double() - rec[kk].double()).abs().max().item() / rec[kk].abs().max().item())
        # (the critics the G step differentiates through have taken 9 - 10 Adam steps of lr * g / (|g| + eps): the elements whose
        # gradient is within rounding of zero have stepped +-lr either way, and the G-step gradient sees those critics)
        print("bf16x6 loop at D = %d: worst G-step gradient element error %.2e of its tensor's scale" % (D, worst))
        for i, (k, p) in enumerate(d["model_G"].named_parameters()):
            GU.compact_close(p.grad.detach().float().cpu(), LU.compact_record(g, "gstep_grad__", k), 100 + i, 1e-7, 1.5e-2, k)
        for key, prefix, steps in (("model_d3d", "final_d3__", 10), ("model_d2d", "final_d2__", 10), ("model_G", "final_G__", 1)):
            for i, (k, p) in enumerate(d[key].named_parameters()):
                rec = LU.compact_record(g, prefix, k)
                got = GU.compact(p.detach().float().cpu() - init[key][k], 100 + i)
                kk = "full" if "full" in rec else "sample"
                e = (got[kk].double() - rec[kk].double()).abs()
                assert e.max().item() <= 1.05 * 2 * steps * 1e-4, (key, k, e.max().item())
                if e.numel() >= 64:
                    # (D = 1000: 2.008e-5 on special_KCS_block1.fc1.weight in one run of seven, below 2e-5 in the others -- the bias gradients' column sums add their
                    # row slabs with atomics, so near-zero gradient elements step +-lr differently from run to run; bound with room)
                    assert torch.quantile(e, 0.98).item() <= (2e-5 if D == 256 else 3e-5), (key, k, torch.quantile(e, 0.98).item())
        return
    # ---- bf16: the arithmetic bench.py times ------------------------------------------------------------------------
    for name, rr in ref.items():
        got = torch.tensor(w.s[name], dtype=torch.float64)
        assert got.shape == rr.shape, name
        assert maxabs(got, rr) <= 5e-2 * max(1.0, rr.abs().max().item()), (name, maxabs(got, rr))
    # generated pairs: the bf16 trunk's poses (3e-2 m of +-10 m roots is what a bf16 head gives; the FK itself is fp32)
    # (the projection divides by the camera depth: a pose next to the camera plane turns centimetres into units, so the 2D pairs are
    # compared by quantile)
    e2 = (torch.cat(p2).detach().double().cpu() - g["buf_p2"].double()).abs().reshape(-1)
    assert maxabs(torch.cat(p3), g["buf_p3"]) <= 0.15 and torch.quantile(e2, 0.99).item() <= 0.15, torch.quantile(e2, 0.99).item()
    cs = torch.nn.functional.cosine_similarity
    worst = 1.0
    for i, (k, p) in enumerate(d["model_G"].named_parameters()):
        rec = LU.compact_record(g, "gstep_grad__", k)
        kk = "full" if "full" in rec else "sample"
        a, b = GU.compact(p.grad.detach().float().cpu(), 100 + i)[kk].double(), rec[kk].double()
        if b.abs().max() > 0:
            c = cs(a, b, dim=0).item()
            worst = min(worst, c)
            assert c > 0.9, (k, c)
            # (D = 1000: measured 0.17 on the 128-column input layer -- a bf16 trunk of K = 1000 layers under ten-step-old bf16 critics)
            assert abs(a.norm().item() / b.norm().item() - 1.0) <= (0.15 if D == 256 else 0.3), (k, a.norm().item(), b.norm().item())
    # ten Adam steps per critic: where the reference moved a weight by (nearly) the full 10 x lr, the bf16 run moved it the same way
    for key, prefix in (("model_d3d", "final_d3__"), ("model_d2d", "final_d2__")):
        agree, total = 0, 0
        for i, (k, p) in enumerate(d[key].named_parameters()):
            rec = LU.compact_record(g, prefix, k)
            kk = "full" if "full" in rec else "sample"
            got = GU.compact(p.detach().float().cpu() - init[key][k], 100 + i)[kk].double()
            big = rec[kk].double().abs() >= 8e-4
            agree += int((torch.sign(got[big]) == torch.sign(rec[kk].double()[big])).sum())
            total += int(big.sum())
        assert total > 1000 and agree >= 0.97 * total, (key, agree, total)
    print("bf16 loop at D = %d: worst G-step gradient cosine %.4f" % (D, worst))


def test_video_loop_vs_reference(M, golden):
    g = golden("video_loop_D32")
    iters, B, R = g["real3d"].shape[0], g["real3d"].shape[1], g["real3d"].shape[2]
    args = _args(batch_size=B, single_or_multi_train_mode="multi", architecture="3,3", single_dis_warmup_epoch=0,
                 GAN_video_playback_input=True, flip_GAN_model_input=True, GAN_3d_motion_loss_weight=1.0,
                 GAN_2d_motion_loss_weight=1.0)
    fk = M.fkm.Forward_Kinematics_DH_Model(args, ["S1"], None)
    d = M.train.video_mode_my_get_poseFk_model(args, None, fk, R)
    names = dict(G="model_G", d3="model_d3d", d2="model_d2d", m3="model_motion_d3d", m2="model_motion_d2d")
    for tag, sd in LU.video_state_dicts(g, R=R).items():
        d[names[tag]].load_state_dict(sd)
        d[names[tag]].precision = "bf16x6"
    al = LU.video_alphas(g)
    per = len(al) // iters
    w, s = Writer(), Summary(epoch=1)
    p3, p2 = [], []
    for i in range(iters):
        last = i == iters - 1
        draws = M.train.Draws(noise=[g["noise"][i]] + ([g["noise"][iters]] if last else []),
                              scaler=[g["scaler"][i]] + ([g["scaler"][iters]] if last else []),
                              alpha=al[per * i:per * (i + 1)])
        cam = (g["cam_quat"][i].tolist(), g["cam_trans"][i].tolist(), g["buf_cam"][i * B, 0].tolist())
        r = M.video.video_gan_iteration(args, d, g["real3d"][i], g["cam_param"], g["real2d"][i], ["S1"], s, w,
                                        do_g_step=last, camera=cam, draws=draws)
        assert not any(draws.q.values()), "recorded draws left over"
        p3.append(r["pos_3d_cam"]); p2.append(r["pos_2d"])
        s.train_iter_num += 1
    pairs_close(p3, p2, g)
    scalars_close(w, g, 3e-4)
    grads_close(d["model_G"], g, 3e-3)
    worst = {t: weights_close(d[names[t]], g, "final_%s__" % t, 1 if t == "G" else (10 if t in ("d3", "d2") else 20))
             for t in names}
    print("video loop: worst weight errors", {k: "%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("tag", ["m3", "m2"])
def test_motion_critic_step_vs_reference(M, golden, tag):
    """one critic step of each motion critic in the mode the video loop uses for it (M3: penalty over B clips;
    M2: penalty over B*R frames) -- scalars, gradients before Adam, weights after it"""
    from dhaug_amd.models_Fk_GAN import Fk_discriminator as dis
    g = golden("motion_step_%s_D32" % tag)
    B, R = 8, 9
    args = _args(batch_size=B, single_or_multi_train_mode="multi", architecture="3,3")
    cls = dis.Video_motion_Fk_3D_Discriminator if tag == "m3" else dis.Video_motion_Fk_2D_Discriminator
    net = cls("cuda", args, R)
    net.load_state_dict(GU.seeded_state_dict(LU.motion_shapes(32, R)[0 if tag == "m3" else 1], int(g["weight_seed"])))
    net.precision = "bf16x6"
    net = net.cuda()
    opt = M.train.FusedAdam(net.parameters(), lr=1e-4, betas=(0.5, 0.9))
    W, C = M.train.train_Fk_discriminator(net, g["real"].cuda(), g["fake"].cuda(), Summary(), None, "motion_" + tag, opt,
                                          args, dis_mode="motion" if tag == "m3" else "single", alpha=g["alpha"].cuda())
    assert torch.isfinite(W).item() and torch.isfinite(C).item()
    assert abs(W.item() - g["Wasserstein_D"].item()) <= 2e-5
    assert abs(C.item() - g["D_cost"].item()) <= 2e-4 * max(1.0, abs(g["D_cost"].item()))
    for k, p in net.named_parameters():
        ref = g["grad__" + k]
        assert maxabs(p.grad, ref) <= 2e-5 + 5e-4 * ref.abs().max().item(), (k, maxabs(p.grad, ref))
        assert maxabs(p, g["new__" + k]) <= 1.05e-4, k
        well = ref.abs() > max(1e-3 * ref.abs().max().item(), 1e-7)
        if well.any():
            assert maxabs(p.detach().cpu()[well], g["new__" + k][well]) <= 3e-6, k


@pytest.mark.parametrize("tag", ["m3", "m2"])
def test_motion_critic_step_vs_reference_at_dense_dim_1000(M, golden, tag):
    """The video path's TRAINING kernels at the width of the reference's README video command (DenseDim 1000: the 1000-wide NT
    layers, the wide grouped weight-gradient contractions, adam_nt) against the reference's own train_Fk_discriminator on B = 128
    clips (tests/golden/make_golden_loops.py motion_step_D1000; compact records): (1) in the fp32-grade arithmetic at the golden
    tolerances of the DenseDim-32 / 256 step tests; (2) in the TIMED bf16 arithmetic element-wise against the oracle's bf16
    emulation (<= 5e-2 of EVERY element of a weight gradient's scale, biases 1e-1), whose fp32 form test_oracle_loops.py holds to the same
    fixture on CPU."""
    from dhaug_amd.models_Fk_GAN import Fk_discriminator as dis
    from oracle import dhaug_oracle as O
    g = golden("motion_step_%s_D1000" % tag)
    B, R, D = 128, 9, 1000
    assert g["real"].shape[0] == B * R
    args = _args(batch_size=B, single_or_multi_train_mode="multi", architecture="3,3", video_Dis_DenseDim_3D=D, video_Dis_DenseDim_2D=D)
    cls = dis.Video_motion_Fk_3D_Discriminator if tag == "m3" else dis.Video_motion_Fk_2D_Discriminator
    sd = GU.seeded_state_dict(LU.motion_shapes(D, R)[0 if tag == "m3" else 1], int(g["weight_seed"]))
    rec = lambda kind, k: {part: g["%s__%s__%s" % (kind, part, k)] for part in ("full", "sample", "proj") if "%s__%s__%s" % (kind, part, k) in g}

    def run(prec):
        net = cls("cuda", args, R)
        net.load_state_dict(sd)
        net.precision = prec
        net = net.cuda()
        opt = M.train.FusedAdam(net.parameters(), lr=1e-4, betas=(0.5, 0.9))
        W, C = M.train.train_Fk_discriminator(net, g["real"].cuda(), g["fake"].cuda(), Summary(), None, "motion_" + tag, opt,
                                              args, dis_mode="motion" if tag == "m3" else "single", alpha=g["alpha"].cuda())
        return (W.item(), C.item(), {k: p.grad.detach().float().cpu() for k, p in net.named_parameters()},
                {k: p.detach().float().cpu() for k, p in net.named_parameters()})
    W, C, grads, params = run("bf16x6")
    assert abs(W - g["Wasserstein_D"].item()) <= 2e-5 and abs(C - g["D_cost"].item()) <= 2e-4 * max(1.0, abs(g["D_cost"].item()))
    flips = 0
    for i, k in enumerate(sd):
        # (B = 128 clips: a handful of the step's ~1e7 pre-activations lie within fp32 rounding of zero -- golden_util.compact_close_but_flips)
        flips += GU.compact_close_but_flips(grads[k], rec("grad", k), 100 + i, 2e-6, 5e-4, k)
        ref, got = rec("delta", k), GU.compact(params[k] - sd[k], 100 + i)
        key = "full" if "full" in ref else "sample"
        gref = rec("grad", k)[key]
        ggot = GU.compact(grads[k], 100 + i)[key]
        gtol = 2e-6 + 5e-4 * gref.abs().max().item()                 # (the gradient comparison's own tolerance)
        # Adam's first step is lr * g / (|g| + eps), sign-like: the stepped weights are compared where the reference's gradient is at
        # least twice the gradient tolerance away from zero (at B = 128 the bias gradients are ~5e-4: 1e-3 of that is below the
        # tolerance), and not on an element a flipped unit has moved
        well = gref.abs() > max(1e-3 * gref.abs().max().item(), 1e-7, 2 * gtol)
        well &= (ggot.double() - gref.double()).abs() <= gtol
        if well.any():
            assert (got[key].double() - ref[key].double())[well].abs().max().item() <= 3e-6, k
        assert (got[key].double() - ref[key].double()).abs().max().item() <= 2.05e-4, k
    print("bf16x6 %s step at DenseDim 1000: %d recorded gradient elements beyond the fp32-grade bound (flipped units)" % (tag, flips))
    assert flips <= 12
    # the timed arithmetic against the oracle's bf16 emulation (same rounding points: operands, stored activations, cotangents)
    Wb, Cb, gb, _ = run("bf16")
    fwd = (lambda x, p: O.motion_d3_forward(x, p, R, precision="bf16")) if tag == "m3" else (lambda x, p: O.motion_d2_forward(x, p, R, precision="bf16"))
    rows = B if tag == "m3" else B * R
    net = O.Net(sd, fwd)
    net.zero_grad()
    gp = O.gradient_penalty(net, g["real"].reshape(rows, -1), g["fake"].reshape(rows, -1), g["alpha"])
    lr_, lf_ = net(g["real"]).mean(), net(g["fake"]).mean()
    (lf_ - lr_ + gp).backward()
    print("bf16 %s step: W %.6g / oracle %.6g, D_cost %.6g / oracle %.6g (gp %.6g)" % (tag, Wb, (lr_ - lf_).item(), Cb, (lf_ - lr_ + gp).item(), gp.item()))
    assert abs(Wb - (lr_ - lf_).item()) <= 3e-3 * max(1.0, abs(Wb)) and abs(Cb - (lf_ - lr_ + gp).item()) <= 2e-2 * max(1.0, abs(Cb))
    # Element-wise bound: 5e-2 of a weight gradient's scale, 1e-1 for biases -- for EVERY element (the DenseDim-256 step's 2e-2 / 4e-2
    # with four times the contraction length: measured 4.6e-2 (M3) / 2.4e-2 (M2) at worst on weights, ten to twenty elements in a
    # million over 2e-2; 7.9e-2 / 6.8e-2 on a bias, a residue of the -1/B | +1/B cancellation).  (Round 5's
    # fixture had B = 16 clips: one unit whose pre-activation sat within bf16 rounding of zero, masked on one side in the kernels and
    # on the other in the emulation, moved its gradient row by up to 1 / 16, and the test allowed three such units per tensor up to
    # 2e-1.  At B = 128 a flipped (row, unit) weighs 1 / 128: the allowance is gone.)
    worst = {1: 0.0, 2: 0.0}
    for k, r in net.grads().items():
        scale = r.abs().max().item()
        if scale == 0.0:
            assert gb[k].abs().max().item() == 0.0, k
            continue
        err = (gb[k].double() - r.double()).abs() / scale
        e = err.max().item()
        worst[r.dim()] = max(worst[r.dim()], e)
        assert e <= (5e-2 if r.dim() == 2 else 1e-1), (k, e, scale, (err > 2e-2).double().mean().item())
    print("bf16 %s step at DenseDim 1000 vs bf16-emulated oracle: worst element error %.2e (weights) / %.2e (biases) of scale"
          % (tag, worst[2], worst[1]))


@pytest.mark.parametrize("tag", ["m3", "m2"])
def test_motion_critic_step_branch_layers_grouped_equals_layer_by_layer(M, tag, monkeypatch):
    """DenseDim 1000, bf16: the layers of a motion critic's four / two branches at the same depth as ONE launch each
    (critic_step._layer_major, dhaug_gemm_bf16_group) against one launch per layer -- same kernel body, same operands: scalars,
    gradients and the weights after Adam bit for bit"""
    from dhaug_amd import critic_step as CS
    from dhaug_amd.models_Fk_GAN import Fk_discriminator as dis
    B, R, D = 96, 9, 1000
    args = _args(batch_size=B, single_or_multi_train_mode="multi", architecture="3,3", video_Dis_DenseDim_3D=D, video_Dis_DenseDim_2D=D)
    cls = dis.Video_motion_Fk_3D_Discriminator if tag == "m3" else dis.Video_motion_Fk_2D_Discriminator
    gen = torch.Generator().manual_seed(5)
    w = 48 if tag == "m3" else 32
    real = torch.randn(B, R, w, generator=gen) * 0.3
    fake = real + 0.05 * torch.randn(B, R, w, generator=gen)
    alpha = torch.rand(B if tag == "m3" else B * R, 1, generator=gen)
    res = []
    for grouped in (True, False):
        monkeypatch.setattr(CS, "NT_GROUP", grouped)
        torch.manual_seed(7)
        net = cls("cuda", args, R)
        net.precision = "bf16"
        net = net.cuda()
        opt = M.train.FusedAdam(net.parameters(), lr=1e-4, betas=(0.5, 0.9))
        W, C = M.train.train_Fk_discriminator(net, real.cuda(), fake.cuda(), Summary(), None, "motion_" + tag, opt, args,
                                              dis_mode="motion" if tag == "m3" else "single", alpha=alpha.cuda())
        res.append((W.item(), C.item(), opt.flat_grad.clone(), opt.flat_param.clone()))
    a, b = res
    assert a[0] == b[0] and a[1] == b[1] and torch.isfinite(a[2]).all()
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


@pytest.mark.parametrize("tag", ["m3", "m2"])
@pytest.mark.parametrize("grouped", [True, False])
def test_motion_critic_step_reads_no_unwritten_memory(M, tag, grouped, monkeypatch):
    """DenseDim 1000 is not a multiple of 16: the cotangent of a motion critic's concatenation is handed to the branches as 1000-wide
    column blocks that the backward GEMMs read 1008 wide (against zero columns of the weights' operand copy) -- the last row of the
    last block used to be read 16 bytes beyond the allocation, and NaN x 0 = NaN (found in round 5; critic_step._Bf16Math.empty_blocks).
    With every torch.empty buffer pre-filled with NaN / a huge value the step gives the same bits as without, in both launch forms."""
    from dhaug_amd.models_Fk_GAN import Fk_discriminator as dis
    from dhaug_amd import critic_step as CS
    B, R, D = 16, 9, 1000
    monkeypatch.setattr(CS, "NT_GROUP", grouped)
    args = _args(batch_size=B, single_or_multi_train_mode="multi", architecture="3,3", video_Dis_DenseDim_3D=D, video_Dis_DenseDim_2D=D)
    cls = dis.Video_motion_Fk_3D_Discriminator if tag == "m3" else dis.Video_motion_Fk_2D_Discriminator
    sd = GU.seeded_state_dict(LU.motion_shapes(D, R)[0 if tag == "m3" else 1], 77)
    gen = torch.Generator().manual_seed(9)
    w = 48 if tag == "m3" else 32
    real = (torch.randn(B, R, w, generator=gen) * 0.3).cuda()
    fake = (real.cpu() + 0.05 * torch.randn(B, R, w, generator=gen)).cuda()
    alpha = torch.rand(B if tag == "m3" else B * R, 1, generator=gen).cuda()

    def run():
        net = cls("cuda", args, R)
        net.load_state_dict(sd)
        net.precision = "bf16"
        net = net.cuda()
        opt = M.train.FusedAdam(net.parameters(), lr=1e-4, betas=(0.5, 0.9))
        W, C = M.train.train_Fk_discriminator(net, real, fake, Summary(), None, "motion_" + tag, opt, args,
                                              dis_mode="motion" if tag == "m3" else "single", alpha=alpha)
        return W.item(), C.item(), opt.flat_grad.clone(), opt.flat_param.clone()
    ref = run()
    assert torch.isfinite(ref[2]).all()
    real_empty, real_empty_like = torch.empty, torch.empty_like
    for poison in (float("nan"), 3.0e38):
        def fill(t):
            if t.is_cuda and t.numel():
                if t.dtype.is_floating_point:
                    t.fill_(poison)
                else:
                    t.view(torch.uint8).fill_(255)
            return t
        monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(real_empty(*a, **k)))
        monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(real_empty_like(*a, **k)))
        got = run()
        monkeypatch.setattr(torch, "empty", real_empty)
        monkeypatch.setattr(torch, "empty_like", real_empty_like)
        assert got[0] == ref[0] and got[1] == ref[1], (tag, poison, got[:2], ref[:2])
        assert torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3]), (tag, poison)


# ------------------------------------------------------------------------------- BASELINE configs[4] widths (DenseDim 1000)
def _video_nets(M, B, R, D, prec):
    from dhaug_amd.function_aug.config import synth_args
    args = synth_args(B, D, single_or_multi_train_mode="multi", architecture="3,3", video_Dis_DenseDim_3D=D,
                      video_Dis_DenseDim_2D=D, single_dis_warmup_epoch=0)
    fk = M.fkm.Forward_Kinematics_DH_Model(args, ["S1"], None)
    d = M.train.video_mode_my_get_poseFk_model(args, None, fk, R)
    for k, m in d.items():
        if k.startswith("model"):
            m.precision = prec
    return args, d


def test_video_D1000_forward_vs_reference(M, golden):
    """the video generator and the four critics at DenseDim 1000 (layer-by-layer: the fused programs cover 64/128/256) in the
    fp32-grade arithmetic against the reference's outputs; the bf16 default is measured against the logit scale"""
    g = golden("video_D1000")
    R, D, B = 9, 1000, g["z"].shape[0]
    args, d = _video_nets(M, B, R, D, "bf16x6")
    sG, s3, s2, sm3, sm2 = (int(v) for v in g["seeds"])
    m3s, m2s = LU.motion_shapes(D, R)
    for key, shapes, seed in (("model_G", GU.shapes_generator(D, frames=R), sG), ("model_d3d", GU.shapes_d3(D), s3),
                              ("model_d2d", GU.shapes_d2(D), s2), ("model_motion_d3d", m3s, sm3), ("model_motion_d2d", m2s, sm2)):
        d[key].load_state_dict(GU.seeded_state_dict(shapes, seed))
    G = d["model_G"]
    rel = lambda a, b: ((a.detach().double().cpu() - b.double()).abs() / b.double().abs().clamp_min(0.1 * b.double().abs().mean())).max().item()
    with torch.no_grad():
        G.GAN_generator_get_bone_length(g["real16"].cuda())
        fake = G(g["z"].cuda(), bone_len_scaler=g["scaler"])
        assert fake.shape == (B, R, 48) and maxabs(fake, g["fake"]) <= 3e-5      # roots up to +-10 m; K = 1000 dot products
        outs = dict(d3=d["model_d3d"](g["x3"].cuda()), d2=d["model_d2d"](g["x2"].cuda()),
                    m3=d["model_motion_d3d"](g["x3"].cuda()), m2=d["model_motion_d2d"](g["x2"].cuda()))
        for k, v in outs.items():
            assert rel(v, g["logit_" + k]) <= 1e-4, (k, rel(v, g["logit_" + k]))
        # module precision "f16x3" at this width: no fused program applies, the layers run the SAME arithmetic (IEEE-half pairs, three
        # product terms) as GEMMs on the ping-pong tiles (dhaug_gemm_f16x3; the narrow layers in "bf16x6") -- the tolerance again
        for k, m in d.items():
            if k.startswith("model"):
                m.precision = "f16x3"
        fake3 = G(g["z"].cuda(), bone_len_scaler=g["scaler"])
        assert maxabs(fake3, g["fake"]) <= 3e-5
        outs3 = dict(d3=d["model_d3d"](g["x3"].cuda()), d2=d["model_d2d"](g["x2"].cuda()),
                     m3=d["model_motion_d3d"](g["x3"].cuda()), m2=d["model_motion_d2d"](g["x2"].cuda()))
        for k, v in outs3.items():
            print("f16x3 layer path at DenseDim 1000: %s logits %.2e rel (bf16x6: %.2e)" % (k, rel(v, g["logit_" + k]), rel(outs[k], g["logit_" + k])))
            assert rel(v, g["logit_" + k]) <= 1e-4, (k, rel(v, g["logit_" + k]))
            assert not torch.equal(v, outs[k]), k                               # (it IS another arithmetic than bf16x6)
        for k, m in d.items():
            if k.startswith("model"):
                m.precision = "bf16"
        for k, net, x in (("d3", d["model_d3d"], g["x3"]), ("d2", d["model_d2d"], g["x2"]), ("m3", d["model_motion_d3d"], g["x3"]),
                          ("m2", d["model_motion_d2d"], g["x2"])):
            ref = g["logit_" + k]
            assert maxabs(net(x.cuda()), ref) <= 8e-2 * ref.abs().max().item(), k


def test_video_full_size_iteration_properties(M):
    """BASELINE configs[4] on one GPU: B = 512 clips x R = 9 frames, DenseDim 1000, motion critics, playback and flip on.
    Two iterations (the second with the G step): finite scalars, every network moves by at most (steps x lr), the generated
    pairs have the epoch buffer's layout; a second replica from the same seed reports the same Wasserstein distances."""
    from dhaug_amd import ops
    B, R, D = 512, 9, 1000
    cam = ([0.5, 0.5, -0.5, 0.5], [0.0, 0.0, 5.0], [2.3, 2.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    res = []
    for rep in range(2):
        torch.manual_seed(123)
        args, d = _video_nets(M, B, R, D, "bf16")
        before = {k: [p.detach().clone() for p in m.parameters()] for k, m in d.items() if k.startswith("model")}
        a, bl, rt = GU.synth_fk_inputs(B * R, 5)
        world = ops.fk_forward((a * 0.25).cuda(), bl.cuda(), (rt * 0.2).cuda())
        c3, p2 = ops.world_to_camera_project(world, *cam)
        cp = torch.zeros(B, 16); cp[:, 9:13] = torch.tensor(cam[0]); cp[:, 13:16] = torch.tensor(cam[1])
        s = Summary(epoch=10)
        out = None
        for it in range(2):
            out = M.video.video_gan_iteration(args, d, c3.reshape(B, R, 16, 3), cp, p2.reshape(B, R, 16, 2), ["S1"], s, None,
                                              do_g_step=(it == 1), camera=cam)
        torch.cuda.synchronize()
        vals = {k: (out[k][0].item(), out[k][1].item()) for k in ("d3", "m3", "d2", "m2")}
        assert all(torch.isfinite(torch.tensor(v)).all() for v in vals.values()) and torch.isfinite(out["G_cost"]).item()
        assert out["pos_3d_cam"].shape == (B, R, 16, 3) and out["pos_2d"].shape == (B, R, 16, 2)
        for k, ps in before.items():
            steps = 1 if k == "model_G" else (4 if k in ("model_d3d", "model_d2d") else 8)
            moved = max((p.detach() - q).abs().max().item() for p, q in zip(d[k].parameters(), ps))
            assert 0 < moved <= 1.3e-4 * steps, (k, moved)          # (bias-corrected early Adam steps reach ~1.1 lr)
        res.append(vals)
        del d, before
        torch.cuda.empty_cache()
    for k in res[0]:
        assert abs(res[0][k][0] - res[1][k][0]) <= 2e-3 * max(1.0, abs(res[0][k][0])), (k, res[0][k], res[1][k])


def test_full_size_iteration_with_generator_step(M):
    """BASELINE configs[2] end to end: ONE gan_iteration at B = 65 536, D = 256 in the throughput arithmetic INCLUDING the G
    step (2 + 2 critic steps, sampling pass, explicit generator step): everything finite, every network moves by at most
    its number of Adam steps x lr, and the iteration is reproducible (same seed -> same costs and same weights: no atomics
    are left on this path at this size)."""
    from dhaug_amd.common.camera import camera_params9
    from dhaug_amd.common.h36m_dataset import h36m_cameras_extrinsic_params, h36m_cameras_intrinsic_params
    from dhaug_amd import ops
    B, D = 65536, 256
    args = _args(batch_size=B, Gen_DenseDim=D, Dis_DenseDim_3D=D, Dis_DenseDim_2D=D)
    ext = h36m_cameras_extrinsic_params["S1"][0]
    cam = ([float(v) for v in ext["orientation"]], [float(v) / 1000.0 for v in ext["translation"]],
           camera_params9(h36m_cameras_intrinsic_params[0]))
    g = torch.Generator().manual_seed(3)
    ang = (torch.randn(B, 37, generator=g) * 40).clamp(-180, 180).cuda()
    bl = (torch.rand(B, 15, generator=g) * 0.4 + 0.1).cuda()
    world = ops.fk_forward(ang, bl, (torch.randn(B, 3, generator=g) * 0.3).cuda())
    real_cam, real_2d = ops.world_to_camera_project(world, *cam)
    cp = torch.zeros(B, 16, device="cuda")
    cp[:, 9:13] = torch.tensor(cam[0], device="cuda"); cp[:, 13:16] = torch.tensor(cam[1], device="cuda")

    def run():
        torch.manual_seed(77)
        fk = M.fkm.Forward_Kinematics_DH_Model(args, ["S1"], None)
        d = M.train.my_get_poseFk_model(args, None, fk)
        before = {k: d[k].flat_param.clone() for k in ("optimizer_G", "optimizer_d3d", "optimizer_d2d")}
        draws = M.train.ConstDraws(scaler=[(torch.randint(-200, 200, (B, 8), generator=torch.Generator().manual_seed(5)) / 1000.0).cuda()])
        r = M.train.gan_iteration(args, d, real_cam, cp, real_2d, ["S1"], None, None, do_g_step=True, camera=cam, draws=draws)
        return d, before, r

    d, before, r = run()
    for k in ("Wasserstein_D_3D", "D_cost_3D", "Wasserstein_D_2D", "D_cost_2D", "G_cost"):
        assert torch.isfinite(r[k]).item(), k
    assert torch.isfinite(r["pos_3d_cam"]).all() and torch.isfinite(r["pos_2d"]).all()
    for k, steps in (("optimizer_G", 1), ("optimizer_d3d", 2), ("optimizer_d2d", 2)):
        moved = (d[k].flat_param - before[k]).abs()
        assert torch.isfinite(d[k].flat_param).all() and int(d[k].step_dev.item()) == steps
        assert moved.max().item() <= steps * 1.1e-4, (k, moved.max().item())   # (Adam's 2nd step can exceed lr by a few %: m / sqrt(v) with beta 0.5 / 0.9)
        assert (moved > 0).float().mean().item() > 0.5, k          # (the step reaches the network)
    d2, _, r2 = run()
    for k in ("Wasserstein_D_3D", "D_cost_3D", "Wasserstein_D_2D", "D_cost_2D", "G_cost"):
        assert abs(r2[k].item() - r[k].item()) <= 1e-6 * max(1.0, abs(r[k].item())), k
    for k in ("optimizer_G", "optimizer_d3d", "optimizer_d2d"):
        assert (d2[k].flat_param - d[k].flat_param).abs().max().item() <= 1e-7, k
