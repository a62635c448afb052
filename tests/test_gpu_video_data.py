"""The device-resident video loader on the GPU (dhaug_clip_gather through the C-ABI): bit for bit the reference's batches
(tests/golden/video_data.npz, recorded from the reference's own GAN_video_ChunkedGenerator / video_mode_dataloader_update),
every output element written at H36M scale, and a video GAN epoch fed by it equal to the same epoch fed numpy batches."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from test_video_data_loader import CONFIGS, LEFT, RIGHT, loader, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    dhaug_amd._lib.lib()
    from dhaug_amd.models_Fk_GAN import video_mode_operate
    return video_mode_operate


@pytest.fixture(scope="module")
def G():
    z = np.load(os.path.join(ROOT, "tests", "golden", "video_data.npz"))
    return {k: z[k] for k in z.files}


def collect(gen, n=None):
    out = []
    for i, b in enumerate(gen.next_epoch()):
        if n is not None and i == n:
            break
        out.append(b)
    cat = lambda k: None if out[0][k] is None else torch.cat([b[k] for b in out]).cpu().numpy()
    return cat(0), cat(1), cat(2), [b[2].shape[0] for b in out]


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_batches_equal_the_reference_bit_for_bit(V, G, tag):
    """the loader over the reference's post-swap buffers yields the reference's batches exactly: indexing, edge padding,
    causal shift, flip (negated x, swapped joints, camera columns 2 / 7) and the endless run across an epoch boundary"""
    g = loader(V, G, tag)
    n = len(G[tag + "_bsizes"])
    cam, p3, p2, sizes = collect(g, n)
    assert sizes == list(G[tag + "_bsizes"])
    for b in (cam, p3, p2):
        assert b is None or b.dtype == np.float32
    assert np.array_equal(p3.view(np.int32), G[tag + "_b3d"].view(np.int32))
    assert np.array_equal(p2.view(np.int32), G[tag + "_b2d"].view(np.int32))
    if tag == "end":
        assert cam is None
    else:
        assert np.array_equal(cam.view(np.int32), G[tag + "_bcam"].view(np.int32))


def test_batches_are_fresh_device_tensors(V, G):
    g = loader(V, G, "a33")
    it = g.next_epoch()
    a, b = next(it), next(it)
    for x, y in zip(a, b):
        assert x.is_cuda and x.dtype == torch.float32 and x.data_ptr() != y.data_ptr()
    assert a[1].shape == (16, 9, 16, 3) and a[2].shape == (16, 9, 16, 2) and a[0].shape == (16, 16)


@pytest.mark.parametrize("tag,arch", [("a33", "3,3"), ("a333", "3,3,3")])
def test_data_update_end_to_end(V, G, tag, arch):
    """video_mode_dataloader_update from the raw sequences under the reference's numpy seed: same template per sequence, so
    the batches match the reference's within the bone-swap bound of test_random_bl_aug_golden (1e-5 m).  2D: the projection
    divides by the depth (3-6 m here) and scales by the focal length (~2.3 in normalised units), so a 1e-5 m error moves a
    keypoint by at most ~2.3e-5 * (1 + |x/z|) / 3 < 2e-5; the bound is 2e-5."""
    L = G["len"]
    data = dict(poses_train=split(G["x"], L), poses_train_2d=[np.zeros((n, 16, 2), np.float32) for n in L],
                actions_train=["a"] * len(L), cams_train=list(G["cam"]))
    np.random.seed(int(G[tag + "_seed"]))
    V.video_mode_dataloader_update(argparse.Namespace(batch_size=16, architecture=arch), data, torch.device("cuda"))
    after = np.random.rand()
    np.random.seed(int(G[tag + "_seed"]))
    for _ in L:
        np.random.choice(5, 1)
    assert after == np.random.rand()                         # exactly one draw per sequence
    g = data["target_GAN_loader"]
    assert np.array_equal(np.array(g.pairs), G[tag + "_pairs"]) and g.pad == CONFIGS[tag]["pad"]
    cam, p3, p2, sizes = collect(g, len(G[tag + "_bsizes"]))
    assert sizes == list(G[tag + "_bsizes"])
    assert np.abs(p3 - G[tag + "_b3d"]).max() <= 1e-5
    assert np.abs(p2 - G[tag + "_b2d"]).max() <= 2e-5
    assert np.array_equal(cam, G[tag + "_bcam"])


def _expected(seq3d, seq2d, off, ln, rec, frames, shift, perm):
    """the batch by torch.index_select over clamped frame indices (computed here, independently of the kernel)"""
    rec = rec.long()
    f = torch.arange(frames, device=rec.device)
    t = (rec[:, 1:2] - shift + f).clamp(min=0)
    t = torch.minimum(t, ln[rec[:, 0]].long().unsqueeze(1) - 1) + off[rec[:, 0]].unsqueeze(1)
    out = []
    for s, C in ((seq3d, 3), (seq2d, 2)):
        x = torch.index_select(s, 0, t.reshape(-1)).reshape(-1, frames, 16, C)
        fl = torch.index_select(x, 2, perm)
        fl[..., 0] = -fl[..., 0]
        out.append(torch.where(rec[:, 3].bool().view(-1, 1, 1, 1), fl, x))
    return out


@pytest.mark.parametrize("R,augment", [(27, True), (243, False)])
def test_h36m_scale_every_element_written(V, R, augment):
    """600 sequences of 150-400 frames, B = 512: every batch of an epoch, written into NaN-filled outputs, equals an
    index_select gather"""
    from dhaug_amd import ops
    rng = np.random.RandomState(R)
    lengths = rng.randint(150, 401, 600)
    T = int(lengths.sum())
    gen = torch.Generator(device="cuda").manual_seed(R)
    seq3d = torch.randn(T, 16, 3, device="cuda", generator=gen)
    seq2d = torch.randn(T, 16, 2, device="cuda", generator=gen)
    cams = torch.randn(600, 16, device="cuda", generator=gen)
    pad = (R - 1) // 2
    g = V.GAN_video_ChunkedGenerator._from_device(512, cams, seq3d, seq2d, lengths, 1, pad=pad, augment=augment,
                                                  kps_left=LEFT, kps_right=RIGHT, joints_left=LEFT, joints_right=RIGHT)
    d = g._device_data()
    _, pairs = g.next_pairs()
    rec = torch.from_numpy(pairs.astype(np.int32)).cuda()
    perm = list(range(16))
    for a, b in zip(LEFT, RIGHT):
        perm[a], perm[b] = b, a
    perm_t = torch.tensor(perm, device="cuda")
    assert g.num_batches == (T * (2 if augment else 1) + 511) // 512
    for b in range(g.num_batches):
        r = rec[b * 512:(b + 1) * 512]
        n = r.shape[0]
        o3 = torch.full((n, R, 16, 3), float("nan"), device="cuda")
        o2 = torch.full((n, R, 16, 2), float("nan"), device="cuda")
        oc = torch.full((n, 16), float("nan"), device="cuda")
        ops.clip_gather(seq3d, seq2d, cams, d["offset"], d["length"], r, R, pad, 0, perm if augment else None,
                        perm if augment else None, out3d=o3, out2d=o2, out_cam=oc)
        e3, e2 = _expected(seq3d, seq2d, d["offset"], d["length"], r, R, pad, perm_t)
        ec = cams[r[:, 0].long()].clone()
        ec[:, [2, 7]] *= torch.where(r[:, 3:4].bool(), -1.0, 1.0)
        assert torch.equal(o3, e3) and torch.equal(o2, e2) and torch.equal(oc, ec), b


def test_video_epoch_fed_by_the_loader_equals_numpy_batches(V, G):
    """video_mode_GAN_solutions_FK_generator (DenseDim 32, B = 8, R = 9, three iterations): the loader's device batches and
    the same batches in the reference's numpy form (float64, host) leave the same weights"""
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model as fkm, model_fk_gan_train as train
    from dhaug_amd.models_Fk_GAN import video_GAN_fun as VG
    from test_gpu_models import _Summary, make_args
    L = G["len"]
    keep = [3, 8]                                          # 9 + 15 frames = 24 clips = three batches of 8
    p3, p2 = split(G["a33_p3"], L), split(G["a33_p2"], L)
    c = list(G["cam"])
    make = lambda: V.GAN_video_ChunkedGenerator(8, [c[i] for i in keep], [p3[i] for i in keep], [p2[i] for i in keep], 1,
                                                pad=4, kps_left=LEFT, kps_right=RIGHT, joints_left=LEFT, joints_right=RIGHT)
    host = [tuple(x.cpu().numpy().astype(np.float64) for x in b) for b in make().next_epoch()]
    assert len(host) == 3 and all(b[1].shape == (8, 9, 16, 3) for b in host)

    class NumpyLoader:
        def next_epoch(self):
            yield from host

    args = make_args(batch_size=8, single_or_multi_train_mode="multi", architecture="3,3", single_dis_warmup_epoch=0,
                     GAN_video_playback_input=True, GAN_3d_motion_loss_weight=1.0, GAN_2d_motion_loss_weight=1.0)
    keys = ("model_G", "model_d3d", "model_d2d", "model_motion_d3d", "model_motion_d2d")

    def run(ld):
        torch.manual_seed(11)
        np.random.seed(11)
        fk = fkm.Forward_Kinematics_DH_Model(args, ["S1"], None)
        d = train.video_mode_my_get_poseFk_model(args, None, fk, 9)
        before = [p.detach().clone() for k in keys for p in d[k].parameters()]
        s = _Summary(epoch=1)
        VG.video_mode_GAN_solutions_FK_generator(args, d, dict(target_GAN_loader=ld), None, s, None, ["S1"])
        assert s.train_iter_num == 3
        after = [p.detach().clone() for k in keys for p in d[k].parameters()]
        return before, after

    b1, a1 = run(make())
    b2, a2 = run(NumpyLoader())
    assert all(torch.equal(x, y) for x, y in zip(b1, b2))
    assert any(not torch.equal(x, y) for x, y in zip(b1, a1))
    assert all(torch.equal(x, y) for x, y in zip(a1, a2))
