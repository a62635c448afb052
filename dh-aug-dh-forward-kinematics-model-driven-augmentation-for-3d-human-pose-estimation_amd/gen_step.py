"""The generator step of both epoch loops (R/models_Fk_GAN/model_fk_gan_train.py:415-484, R/models_Fk_GAN/video_GAN_fun.py:421-566)
as an explicit schedule of kernels -- no autograd graph.

    gen_loss = sum_c  w_c * mean D_c(fake)          (flipped / reversed copies averaged in as the reference does)
    (-gen_loss).backward();  optimizer_G.step()

with the critics frozen.  The critics are piecewise linear behind their input features, so d(-gen_loss)/d(fake) is ONE
backward chain per critic seeded with the constant logit cotangent -w_c / rows (critic_step.py's sweep 2 on the fake rows
only, input layers included), then the transposed feature maps (KCS VJP, frame differences, centring, camera + projection
VJP), the FK tail's reverse mode (dhaug_gen_tail_backward) and the generator trunk's backward chain; the trunk's weight
gradients are one grouped contraction launch.  What the reference's copies contribute:
  * L/R-flipped copies (.detach().clone(), :455,:459): value only -- scored by the fused no-grad programs;
  * frame-reversed copies of the motion critics (video loop, `playback`): value AND gradient (torch.flip is differentiable),
    on the view the reference takes them on ((-1, R, 32) for both the 3D and the 2D clip)."""
import torch

from . import autograd_ops as A
from . import critic_step as CS
from . import ops

NONE, RELU, LRELU = A.ACT_NONE, A.ACT_RELU, A.ACT_LRELU


def _const_seed(rows, value, m, dev):
    return m.seed_operand(torch.full((rows, 1), float(value), dtype=torch.float32, device=dev))


def _branch_value_grad(m, net, X, coef, F=None, fwd=None):
    """X (rows, W) fakes as the critic net (critic_step._BranchNet) takes them -> (logits (rows,1), coef * d mean D / d X fp32):
    forward keeping every activation, then the input-gradient chain of the constant logit cotangent coef / rows -- critic_step's
    sweep 2, branch by branch, on all rows (weights frozen: no weight gradients)."""
    rows, Dw = X.shape[0], net.Dw
    s = fwd() if fwd is not None else net.forward(m, net.feats(X) if F is None else F)
    gcat = net.top_backward(m, _const_seed(rows, coef / rows, m, X.device), s)[3]
    gin = []
    for bi, br in enumerate(net.branches):
        _, a2 = CS.stack_bwd(m, br.blocks, gcat[:, bi * Dw:(bi + 1) * Dw], s["h"][bi], s["y"][bi])
        gin.append(br.first.bwd(m, a2[0], None, NONE, 0.0, out_f32=True))
    return s["logits"], net.input_grad(X, gin)


def _d3_value_grad(m, D, fc, coef):
    """fc (N,48) root-relative fakes -> (logits (N,1), coef * d mean D3 / d fc  (N,48) fp32)"""
    kf, _, fwd = CS.d3_features(m, D, fc, -1 if CS._partial_save(fc.shape[0]) else 0)    # (-1: only masks are read back, the blocks' sign bits)
    return _branch_value_grad(m, CS.d3_net(D), fc, coef, F=[kf, fc], fwd=fwd)


def _d2_value_grad(m, D, x, coef):
    """x (N,32) projections -> (logits, coef * d mean D2 / d x (N,32) fp32)"""
    net = CS.d2_net(D)
    L, sl, N = net.L, D.slope, x.shape[0]
    (d1, d2, d3, d4, dl), logits = net.forward(m, x, -1 if CS._partial_save(N) else 0)
    gzl = L[5].bwd(m, _const_seed(N, coef / N, m, x.device), dl, LRELU, sl)
    gz4 = L[4].bwd(m, gzl, d4, NONE, 0.0)
    gz3 = L[3].bwd(m, gz4, d3, LRELU, sl)
    gz2 = L[2].bwd(m, gz3, d2, LRELU, sl)
    gz1 = L[1].bwd(m, gz2, d1, LRELU, sl, skip=gz3)
    return logits, L[0].bwd(m, gz1, None, NONE, 0.0, out_f32=True)


def _motion_value_grad(m, D, net, x, coef):
    """a motion critic D (net: critic_step.m3_net / m2_net) on clips: x (B*R, w) frames -> (logits (B,1), coef * d mean / d x (B*R, w))"""
    l, g = _branch_value_grad(m, net(D), x.reshape(-1, D.video_frame_num * x.shape[1]), coef)
    return l, g.reshape(x.shape)


CONCURRENT = __import__("os").environ.get("DHAUG_NO_CONCURRENT_CRITICS") is None
_STREAMS = {}


def side_streams(cur, n):
    """the n side streams of `cur` (created on first use; graphs.prepare_streams makes them before a capture)"""
    pool = _STREAMS.setdefault((cur.device.index, cur.cuda_stream), [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream())
    return pool


def _parallel(fns):
    """[fn() for fn in fns], every fn on its own side stream (forked from the current one, joined before returning): the
    critics' value + input-gradient chains are independent of each other and mostly launch-bound at the G step's B rows.
    Tensors that come back were allocated on a side stream and are read on the current one: record_stream tells the
    allocator."""
    if not CONCURRENT or len(fns) < 2:
        return [fn() for fn in fns]
    cur = torch.cuda.current_stream()
    if torch.cuda.is_current_stream_capturing():
        # no stream creation inside a capture, and forks only from the stream the capture was begun on (one level: see
        # graphs.prepare_streams); whatever has no stream runs in line
        from . import critic_step
        pool = _STREAMS.get((cur.device.index, cur.cuda_stream), []) if cur.cuda_stream == critic_step.CAPTURE_ROOT else []
    else:
        pool = side_streams(cur, len(fns))
    out = []
    for i, fn in enumerate(fns):
        if i >= len(pool):
            out.append(fn())
            continue
        st = pool[i]
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            r = fn()
        _record_stream(r, cur)
        out.append(r)
    for st in pool[:len(fns)]:
        cur.wait_stream(st)
    return out


def _record_stream(r, stream):
    """every tensor of a (nested) result: it was allocated on a side stream and will be read on `stream`"""
    if torch.is_tensor(r):
        r.record_stream(stream)
    elif isinstance(r, (tuple, list)):
        for t in r:
            _record_stream(t, stream)
    elif isinstance(r, dict):
        for t in r.values():
            _record_stream(t, stream)


def supported(G, oG, critics):
    """the explicit schedule covers the reference's generators and critics under a FusedAdam bucket, in every arithmetic of
    the layer path"""
    from .models_Fk_GAN.Fk_discriminator import (Fk_2D_Discriminator, Fk_3D_Discriminator, Video_motion_Fk_2D_Discriminator,
                                                 Video_motion_Fk_3D_Discriminator)
    from .models_Fk_GAN.Fk_generator import _GeneratorBase
    from .optim import FusedAdam
    if not isinstance(oG, FusedAdam) or not isinstance(G, _GeneratorBase) or len(critics) not in (2, 4):
        return False
    kinds = (Fk_3D_Discriminator, Fk_2D_Discriminator, Video_motion_Fk_3D_Discriminator, Video_motion_Fk_2D_Discriminator)
    if any(type(c) is not k for c, k in zip(critics, kinds)):
        return False
    ok = ("bf16", "bf16x3", "bf16x6", "f16x3")
    return G.precision in ok and all(c.precision in ok for c in critics) and getattr(G.args, "whether_use_RT", True)


def generator_step(args, G, oG, critics, weights, camera, flip, noise, scaler, frames=1, playback=False):
    """One G step; returns G_cost = -gen_loss (0-dim device tensor).  noise (B,128); scaler: the (B,8) bone-length jitter
    draw or None (drawn on the device like Fk_Generator.forward does)."""
    from .models_Fk_GAN.Fk_generator import graph_precision
    dev = noise.device
    quat, trans, cam9 = camera
    R = frames
    mG = CS.math_for(graph_precision(G.precision))
    oG.zero_grad()
    # ---- forward: trunk (every activation kept), FK tail, camera
    Lp = CS._Lin(G.preprocess[0], RELU)
    blocks = [CS._Block(b) for b in (G.block1, G.block2, G.block3)]
    Lh = CS._Lin(G.deconv_out, NONE)
    z = noise.contiguous().float()
    B = z.shape[0]
    N = B * R
    ys, hs = [Lp.fwd(mG, z)], []
    for blk in blocks:
        h, y = blk.fwd(mG, ys[-1])
        hs.append(h); ys.append(y)
    head = Lh.fwd(mG, ys[-1], out_f32=True)                       # (B, 35 R) fp32
    head2 = head.reshape(N, 35)
    bl = G.boneLength
    if bl.shape[0] != N:
        raise RuntimeError("boneLength has %d rows, the batch needs %d (call GAN_generator_get_bone_length)" % (bl.shape[0], N))
    pre = bool(args.GAN_whether_use_preAngle)
    sc = G._scaler(B, scaler)
    fw = ops.gen_tail_forward(head2, bl, sc, pre)[0]             # (N,16,3) world
    G.train_num += 1
    _, f2d = ops.world_to_camera_project(fw, quat, trans, cam9)
    fc = ops.center_flip(fw, True, False).reshape(N, 48)
    x2 = f2d.reshape(N, 32)
    # ---- critics: value + input gradient of -w * mean D(.) (the L/R-flipped copies halve the weight of the plain ones)
    half = 0.5 if flip else 1.0
    m3d, m2d = CS.math_for(graph_precision(critics[0].precision)), CS.math_for(graph_precision(critics[1].precision))
    jobs = [lambda: _d3_value_grad(m3d, critics[0], fc, -weights[0] * half),
            lambda: _d2_value_grad(m2d, critics[1], x2, -weights[1] * half)]
    wts = [weights[0] * half, weights[1] * half]
    kinds = ["fc", "x2"]
    rev = lambda t: ops.frame_reverse(t.reshape(-1, R * 32), R, 32)
    if len(critics) == 4:
        mm3, mm2 = CS.math_for(graph_precision(critics[2].precision)), CS.math_for(graph_precision(critics[3].precision))
        ph = 0.5 if playback else 1.0
        jobs += [lambda: _motion_value_grad(mm3, critics[2], CS.m3_net, fc, -weights[2] * half * ph),
                 lambda: _motion_value_grad(mm2, critics[3], CS.m2_net, x2, -weights[3] * half * ph)]
        wts += [weights[2] * half * ph, weights[3] * half * ph]
        kinds += ["fc", "x2"]
        if playback:
            # the reference reverses the frames of the clip VIEWED as (-1, R, 32) -- also for the 3D clip: a
            # permutation of the clip's values that is its own transpose
            def rev3_job():
                l, g = _motion_value_grad(CS.math_for(graph_precision(critics[2].precision)), critics[2], CS.m3_net, rev(fc).reshape(N, 48),
                                      -weights[2] * half * ph)
                return l, rev(g).reshape(N, 48)

            def rev2_job():
                l, g = _motion_value_grad(CS.math_for(graph_precision(critics[3].precision)), critics[3], CS.m2_net, rev(x2).reshape(N, 32),
                                      -weights[3] * half * ph)
                return l, rev(g).reshape(N, 32)
            jobs += [rev3_job, rev2_job]
            wts += [weights[2] * half * ph, weights[3] * half * ph]
            kinds += ["fc", "x2"]
    flip_terms = []
    if flip:                                                      # value only (R/...:455-468): fused no-grad programs
        def flip_job():
            with torch.no_grad():
                fcf, x2f = ops.center_flip(fc.reshape(N, 16, 3), False, True), ops.center_flip(x2.reshape(N, 16, 2), False, True)
                t = [(critics[0](fcf), weights[0] * 0.5), (critics[1](x2f), weights[1] * 0.5)]
                if len(critics) == 4:
                    ph2 = 0.5 if playback else 1.0
                    t += [(critics[2](fcf.reshape(-1, 48)), weights[2] * 0.5 * ph2), (critics[3](x2f.reshape(-1, 32)), weights[3] * 0.5 * ph2)]
                    if playback:
                        t += [(critics[2](rev(fcf).reshape(-1, 48)), weights[2] * 0.5 * ph2),
                              (critics[3](rev(x2f).reshape(-1, 32)), weights[3] * 0.5 * ph2)]
            return tuple(l for l, _ in t), [w for _, w in t]
        jobs.append(flip_job)
    res = _parallel(jobs)
    terms = []                                                    # (logits, weight) of every mean in gen_loss
    g_fc = g_x2 = None
    for (l, g), w, kind in zip(res[:len(wts)], wts, kinds):
        terms.append((l, w))
        if kind == "fc":
            g_fc = g if g_fc is None else ops.add_f32(g_fc, g)
        else:
            g_x2 = g if g_x2 is None else ops.add_f32(g_x2, g)
    if flip:
        ls, ws = res[-1]
        terms += list(zip(ls, ws))
    G_cost = ops.weighted_means([t for t, _ in terms], [-w for _, w in terms])          # -gen_loss
    # ---- back through centring, camera + projection, the FK tail
    g_fw = ops.add_f32(ops.center_flip(g_fc.reshape(N, 16, 3), True, False, adjoint=True).reshape(N, 48),
                       ops.world_to_camera_project_backward(fw, quat, trans, cam9, None, g_x2).reshape(N, 48))
    g_head = ops.gen_tail_backward(head2, bl, sc, g_fw, pre).reshape(B, 35 * R)
    # ---- trunk: backward chain + weight gradients (one grouped contraction launch where the shapes allow)
    slot = CS._slot
    gz = Lh.bwd(mG, g_head, ys[-1], RELU, 0.0)                    # cotangent at block3.fc2's pre-activation
    mG.outer(g_head, ys[-1], Lh.N, Lh.K, slot(Lh.W), slot(Lh.b))
    for i in range(len(blocks) - 1, -1, -1):
        gz1, gz_in = blocks[i].bwd(mG, gz, hs[i], ys[i])
        mG.outer(gz, hs[i], blocks[i].fc2.N, blocks[i].fc2.K, slot(blocks[i].fc2.W), slot(blocks[i].fc2.b))
        mG.outer(gz1, ys[i], blocks[i].fc1.N, blocks[i].fc1.K, slot(blocks[i].fc1.W), slot(blocks[i].fc1.b))
        gz = gz_in
    mG.outer(gz, z, Lp.N, Lp.K, slot(Lp.W), slot(Lp.b))
    mG.flush()
    oG.step()
    return G_cost
