"""The posenet data loaders on the GPU (dhaug_clip_gather_windows / dhaug_clip_pair_batch through the C-ABI): bit for bit the
reference's ChunkedGenerator / UnchunkedGenerator batches (tests/golden/video_posedata.npz), equal to the existing gather where the
windows coincide, the fused pair batch equal to the two launches it replaces, multi-pass and all-clamped sizes against an
independent index_select gather, and video_mode_train_posenet / video_mode_evaluate fed by the loaders equal to the same loops fed
the same batches as host numpy.  Every comparison is exact: the kernels copy, negate, permute and subtract once."""
import argparse
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import posetrain_util as PU
import video_posedata_util as U

ROOT = U.ROOT
pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    dhaug_amd._lib.lib()
    from dhaug_amd import ops, optim
    from dhaug_amd.models_Fk_GAN import video_mode_operate
    return argparse.Namespace(ops=ops, optim=optim, V=video_mode_operate)


@pytest.fixture(scope="module")
def G():
    return U.load("video_data.npz")


@pytest.fixture(scope="module")
def P():
    return U.load("video_posedata.npz")


def bits(t):
    return t.cpu().numpy().view(np.int32)


def same_bits(got, want):
    """got: list of device tensors (or None) -> their concatenation equals the recorded array as int32"""
    if got[0] is None:
        return want is None
    return want is not None and np.array_equal(np.concatenate([bits(t.reshape((-1,) + tuple(t.shape[-2:]))) for t in got]),
                                               want.view(np.int32).reshape((-1,) + want.shape[-2:]))


# ------------------------------------------------------------------------------------------------------ 1. fixture parity
@pytest.mark.parametrize("tag", sorted(U.CHUNKED))
def test_chunked_batches_equal_the_reference_bit_for_bit(M, G, P, tag):
    """indexing, edge padding on both sides, causal shift of either sign, the record flip (negated x, swapped joints, camera
    columns 2 / 7), None members, the short last batch, the one-clip batch and the endless run across an epoch boundary"""
    g = U.chunked(M.V, G, tag)
    n = len(P[tag + "_bsizes"])
    out = []
    for i, b in enumerate(g.next_epoch()):
        if i == n:
            break
        out.append(b)
    assert len(out) == n and [b[2].shape[0] for b in out] == list(P[tag + "_bsizes"])
    B, kw = U.CHUNKED[tag]
    for cam, b3, b2 in out:
        assert b2.is_cuda and b2.dtype == torch.float32 and b2.shape[1:] == (kw["chunk_length"] + 2 * kw["pad"], 16, 2)
        assert b3 is None or (b3.dtype == torch.float32 and b3.shape[1:] == (kw["chunk_length"], 16, 3))
    assert same_bits([b[2] for b in out], P[tag + "_b2d"])
    assert same_bits([b[1] for b in out], P.get(tag + "_b3d"))
    cams = [b[0] for b in out]
    if tag == "end":
        assert cams[0] is None and out[0][1] is None and g.state is not None
    else:
        assert np.array_equal(np.concatenate([bits(c) for c in cams]), P[tag + "_bcam"].view(np.int32))
        assert out[0][1].data_ptr() != out[1][1].data_ptr()                       # fresh tensors per batch
    if tag == "c333":
        assert out[-1][2].shape[0] == 1


@pytest.mark.parametrize("tag", sorted(U.UNCHUNKED))
def test_unchunked_batches_equal_the_reference_bit_for_bit(M, G, P, tag):
    g = U.unchunked(M.V, G, tag)
    kw = U.UNCHUNKED[tag]
    m = 2 if kw["augment"] else 1
    out = list(g.next_epoch())
    assert len(out) == len(G["len"])
    for (cam, b3, b2), T in zip(out, G["len"]):
        assert cam.shape == (m, 16) and b3.shape == (m, T, 16, 3) and b2.shape == (m, T + 2 * kw["pad"], 16, 2)
        assert all(t.is_cuda and t.dtype == torch.float32 for t in (cam, b3, b2))
    assert same_bits([b[1] for b in out], P[tag + "_b3d"])
    assert same_bits([b[2] for b in out], P[tag + "_b2d"])
    assert np.array_equal(np.concatenate([bits(b[0]) for b in out]), P[tag + "_bcam"].view(np.int32))
    # without cameras and 3D the members are None, as the reference's zip_longest yields them
    _, _, p2 = U.inputs(G, tag)
    cam, b3, b2 = next(M.V.UnchunkedGenerator(None, None, p2, **kw).next_epoch())
    assert cam is None and b3 is None and torch.equal(b2, out[0][2])


# ------------------------------------------------------------------------------- 2. / 3. against the existing kernels
def _device_case(M, G, tag):
    """(loader, device data, first epoch's record table on the device) of a recorded ChunkedGenerator configuration"""
    g = U.chunked(M.V, G, tag)
    d = g._device_data()
    rec = torch.from_numpy(np.ascontiguousarray(g.next_pairs()[1], dtype=np.int32)).cuda()
    return g, d, rec


@pytest.mark.parametrize("tag", ["aug", "c333"])
def test_equal_windows_are_the_existing_gather(M, G, tag):
    g, d, rec = _device_case(M, G, tag)
    args = (d["seq3d"], d["seq2d"], d["cams"], d["offset"], d["length"], rec)
    old = M.ops.clip_gather(*args, g.frames, g.pad, g.causal_shift, g._perm3d, g._perm2d)
    shift = g.pad + g.causal_shift
    n = rec.shape[0]
    pre = dict(out3d=torch.full((n, g.frames, 16, 3), NAN, device="cuda"), out2d=torch.full((n, g.frames, 16, 2), NAN, device="cuda"),
               out_cam=torch.full((n, 16), NAN, device="cuda"))
    new = M.ops.clip_gather_windows(*args, g.frames, shift, g.frames, shift, g._perm3d, g._perm2d, **pre)
    assert new[1] is pre["out3d"] and new[2] is pre["out2d"] and new[0] is pre["out_cam"]
    for a, b in zip(old, new):
        assert torch.equal(a, b)                                                  # (a NaN left behind is unequal to anything)


def _check_pairs(M, d, rec, windows, perm3d, perm2d, flip, playback):
    """clip_pair_batch into NaN-filled outputs == pair_batch(clip_gather_windows(...)); returns both"""
    _, p3, p2 = M.ops.clip_gather_windows(d["seq3d"], d["seq2d"], None, d["offset"], d["length"], rec, *windows, perm3d, perm2d)
    two = M.ops.pair_batch(p3, p2, flip=flip, playback=playback)
    pre = {k: torch.full_like(v, NAN) for k, v in two.items()}
    one = M.ops.clip_pair_batch(d["seq3d"], d["seq2d"], d["offset"], d["length"], rec, *windows, perm3d, perm2d, flip=flip,
                                playback=playback, out=pre)
    want = {"tgt", "inp"} | ({"tgt_flip", "inp_flip"} if flip else set()) | ({"inp_back"} if playback else set()) \
        | ({"inp_flip_back"} if flip and playback else set())
    assert set(one) == set(two) == want
    for k in want:
        assert one[k] is pre[k] and torch.equal(one[k], two[k]), k
    return one, (p3, p2)


@pytest.mark.parametrize("flip,playback", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("tag", ["aug", "c333"])
def test_fused_pair_batch_equals_the_two_launches(M, G, tag, flip, playback):
    """'aug': the record's flip and the training flip together, chunks of four 3D frames; 'c333': one 3D frame, 27 2D frames"""
    g, d, rec = _device_case(M, G, tag)
    one, (p3, p2) = _check_pairs(M, d, rec, g._windows(), g._perm3d, g._perm2d, flip, playback)
    exp = U.expected_pairs(p3, p2, torch.tensor(U.FLIP_PERM, device="cuda"), flip, playback)
    for k, v in exp.items():
        assert torch.equal(one[k], v), k
    # next_epoch_pairs hands out the same tensors batch by batch
    B = g.batch_size
    for b, batch in enumerate(U.chunked(M.V, G, tag).next_epoch_pairs(flip, playback)):
        for k, v in batch.items():
            assert torch.equal(v, one[k][b * B:(b + 1) * B]), (b, k)
    assert b == g.num_batches - 1


# --------------------------------------------------------------------------------------------------------- 4. multi-pass
def test_multi_pass_batch_every_element_written(M):
    """B = 1024 clips of 243 frames over 600 sequences of 150-400 frames: the gather's capped grid runs
    video_posedata_util.MULTI_GATHER_PASSES (2) passes, the pair batch's MULTI_PAIR_PASSES (2); record flips on.  The gather
    against an index_select gather computed here, the fused pair batch against the two launches and the torch expressions."""
    B, R = U.MULTI_B, U.MULTI_R
    pad = (R - 1) // 2
    rng = np.random.RandomState(R)
    lengths = rng.randint(150, 401, 600)
    T = int(lengths.sum())
    gen = torch.Generator(device="cuda").manual_seed(R)
    seq3d = torch.randn(T, 16, 3, device="cuda", generator=gen)
    seq2d = torch.randn(T, 16, 2, device="cuda", generator=gen)
    cams = torch.randn(600, 16, device="cuda", generator=gen)
    g = M.V.ChunkedGenerator._from_device(B, cams, seq3d, seq2d, lengths, 1, pad=pad, augment=True, **U.LR)
    d = g._device_data()
    pairs = g.next_pairs()[1][:B]
    assert len(pairs) == B and B * (12 + R * 8) > U.QUADS_PER_PASS and B * (1 + R) > U.POSE_FRAMES_PER_PASS
    start, last = pairs[:, 1], lengths[pairs[:, 0]] - 1
    assert (start - pad < 0).any() and (start + pad > last).any() and pairs[:, 3].any() and not pairs[:, 3].all()   # both clamps
    rec = torch.from_numpy(pairs.astype(np.int32)).cuda()
    windows = g._windows()
    assert windows == (1, 0, R, pad)
    perm_t = torch.tensor(U.FLIP_PERM, device="cuda")
    o3 = torch.full((B, 1, 16, 3), NAN, device="cuda")
    o2 = torch.full((B, R, 16, 2), NAN, device="cuda")
    oc = torch.full((B, 16), NAN, device="cuda")
    M.ops.clip_gather_windows(seq3d, seq2d, cams, d["offset"], d["length"], rec, *windows, U.FLIP_PERM, U.FLIP_PERM, out3d=o3,
                              out2d=o2, out_cam=oc)
    e3, e2 = U.expected_windows(seq3d, seq2d, d["offset"], d["length"], rec, *windows, perm_t)
    ec = cams[rec[:, 0].long()].clone()
    ec[:, [2, 7]] *= torch.where(rec[:, 3:4].bool(), -1.0, 1.0)
    assert torch.equal(o3, e3) and torch.equal(o2, e2) and torch.equal(oc, ec)
    one, _ = _check_pairs(M, d, rec, windows, U.FLIP_PERM, U.FLIP_PERM, True, True)
    for k, v in U.expected_pairs(e3, e2, perm_t, True, True).items():
        assert torch.equal(one[k], v), k


# -------------------------------------------------------------------------------------------------- 5. all-clamped sizes
def test_sequences_of_one_and_two_frames(M):
    """pad 13 over sequences of 1 and 2 frames: every frame of every clip is a clamped copy"""
    lengths = [1, 2, 2, 1, 2]
    rng = np.random.RandomState(12)
    p3 = [rng.randn(n, 16, 3).astype(np.float32) for n in lengths]
    p2 = [rng.randn(n, 16, 2).astype(np.float32) for n in lengths]
    cam = [rng.randn(16).astype(np.float32) for _ in lengths]
    perm_t = torch.tensor(U.FLIP_PERM, device="cuda")
    g = M.V.ChunkedGenerator(3, cam, p3, p2, 1, pad=13, causal_shift=1, shuffle=False, augment=True, **U.LR)
    d = g._device_data()
    rec = torch.from_numpy(g.next_pairs()[1].astype(np.int32)).cuda()
    assert rec.shape[0] == 16
    out = list(g.next_epoch())
    e3, e2 = U.expected_windows(d["seq3d"], d["seq2d"], d["offset"], d["length"], rec, 1, 0, 27, 14, perm_t)
    assert torch.equal(torch.cat([b[1] for b in out]), e3) and torch.equal(torch.cat([b[2] for b in out]), e2)
    first = out[0][2][0]                                                          # sequence 0 has one frame: 27 copies of it
    assert torch.equal(first, torch.from_numpy(p2[0]).cuda().expand(27, 16, 2))
    _check_pairs(M, d, rec, g._windows(), g._perm3d, g._perm2d, True, True)
    u = M.V.UnchunkedGenerator(cam, p3, p2, pad=13, causal_shift=-13, augment=True, **U.LR)
    for s, (c, b3, b2) in enumerate(u.next_epoch()):
        n = lengths[s]
        x2, x3 = torch.from_numpy(p2[s]).cuda(), torch.from_numpy(p3[s]).cuda()
        assert torch.equal(b3[0], x3) and b2.shape == (2, n + 26, 16, 2)
        assert torch.equal(b2[0], torch.cat([x2, x2[-1:].expand(26, 16, 2)]))      # pad + shift = 0 in front, 26 behind
        fl = torch.index_select(b2[0], 1, perm_t)
        fl[..., 0] = -fl[..., 0]
        assert torch.equal(b2[1], fl)
        assert torch.equal(c[1, [2, 7]], -c[0, [2, 7]]) and torch.equal(c[0], torch.from_numpy(cam[s]).cuda())


# ------------------------------------------------------------------------------------------------------- 6. end to end
class _HostBatches:
    """the reference's loaders as the loops see them: next_epoch() yielding float64 numpy batches"""

    def __init__(self, batches):
        self.batches = [tuple(None if t is None else t.cpu().numpy().astype(np.float64) for t in b) for b in batches]

    def next_epoch(self):
        yield from self.batches


def test_training_loop_fed_by_the_loader_equals_numpy_batches(M, G):
    """video_mode_train_posenet with PosenetAdam, flip and playback on, B = 13, pad 4 over the fixture's 92 frames: seven batches
    of 13 and one of a single clip, at which the loop stops -> 28 steps.  The loader's fused batches and the same batches handed
    over as float64 numpy leave identical parameters, traces and meters."""
    make = lambda: M.V.ChunkedGenerator(13, *U.inputs(G, "c33"), chunk_length=1, pad=4, **U.LR)
    host = _HostBatches(list(make().next_epoch()))
    assert [b[2].shape[0] for b in host.batches] == [13] * 7 + [1]
    fn = M.V.video_mode_train_posenet

    def run(loader):
        torch.manual_seed(0)
        model = PU.StubPosenet(9).cuda()
        opt = M.optim.PosenetAdam(model.parameters(), lr=PU.LR)
        fn(model, loader, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"), PU.loop_args())
        return {k: v.detach().clone() for k, v in model.state_dict().items()}, fn.last_trace.clone(), dict(fn.last_meters)

    s1, t1, m1 = run(make())
    s2, t2, m2 = run(host)
    assert m1["steps"] == 28 == t1.shape[0]                                      # 7 batches x 4 steps: stopped at the one-clip batch
    assert torch.equal(t1, t2) and m1 == m2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    torch.manual_seed(0)
    init = PU.StubPosenet(9).state_dict()
    assert all(not torch.equal(s1[k].cpu(), init[k]) for k in ("a.weight", "b.weight", "c.weight"))    # and it did train


class _TemporalStub(nn.Module):
    """(m, T + 8, 16, 2) -> (m, T, 16, 3): one temporal convolution over the receptive field of 9"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.conv = nn.Conv1d(32, 48, 9)

    def forward(self, x):
        y = self.conv(x.reshape(x.shape[0], x.shape[1], 32).permute(0, 2, 1))
        return y.permute(0, 2, 1).reshape(x.shape[0], -1, 16, 3)


@pytest.mark.parametrize("flipaug", ["", "_flip"])
def test_evaluation_fed_by_the_loader_equals_numpy_batches(M, G, flipaug):
    """video_mode_evaluate takes UnchunkedGenerator's device batches as they come: the same four numbers as over the same batches
    as host numpy"""
    make = lambda: M.V.UnchunkedGenerator(*U.inputs(G, "u4"), pad=4, causal_shift=0, augment=False, **U.LR)
    host = _HostBatches(list(make().next_epoch()))
    args = argparse.Namespace(architecture="3,3", posenet_name="mulit_farme_videopose")
    net = _TemporalStub().cuda()
    r1 = M.V.video_mode_evaluate(args, make(), net, torch.device("cuda"), flipaug=flipaug, get_pck_auc=True)
    r2 = M.V.video_mode_evaluate(args, host, net, torch.device("cuda"), flipaug=flipaug, get_pck_auc=True)
    assert len(r1) == 4 and all(np.isfinite(v) for v in r1) and tuple(r1) == tuple(r2)
