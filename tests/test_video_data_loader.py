"""CPU checks of the device-resident video loader's host side (no GPU needed): the pair list, the shuffle order and the batch
split equal the reference's (tests/golden/video_data.npz, recorded from the reference's own GAN_video_ChunkedGenerator), and
bad arguments raise before anything is launched."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEFT, RIGHT = [4, 5, 6, 10, 11, 12], [1, 2, 3, 13, 14, 15]
LR = dict(kps_left=LEFT, kps_right=RIGHT, joints_left=LEFT, joints_right=RIGHT)


@pytest.fixture(scope="module")
def V():
    sys.path.insert(0, ROOT)
    from dhaug_amd.models_Fk_GAN import video_mode_operate
    return video_mode_operate


@pytest.fixture(scope="module")
def G():
    z = np.load(os.path.join(ROOT, "tests", "golden", "video_data.npz"))
    return {k: z[k] for k in z.files}


def split(a, lengths):
    return np.split(a, np.cumsum(lengths)[:-1])


def cams(G):
    return list(G["cam"])


# (fixture tag, constructor keywords, batches recorded)
CONFIGS = {
    "a33": dict(chunk_length=1, pad=4, **LR),
    "a333": dict(chunk_length=1, pad=13, **LR),
    "aug": dict(chunk_length=4, pad=2, causal_shift=1, random_seed=5, augment=True, **LR),
    "end": dict(chunk_length=1, pad=1, random_seed=7, endless=True, **LR),
}


def loader(V, G, tag, batch_size=16):
    src = "a333" if tag == "a333" else "a33"
    L = G["len"]
    cam = None if tag == "end" else cams(G)
    return V.GAN_video_ChunkedGenerator(batch_size, cam, split(G[src + "_p3"], L), split(G[src + "_p2"], L), **CONFIGS[tag])


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_pairs_order_and_split_match_the_reference(V, G, tag):
    g = loader(V, G, tag)
    assert np.array_equal(np.array(g.pairs, dtype=np.int64), G[tag + "_pairs"])
    assert all(type(p[3]) is bool for p in g.pairs)
    P = len(g.pairs)
    assert g.num_batches == (P + 15) // 16 and g.num_frames() == g.num_batches * 16 and g.batch_size == 16
    assert g.augment_enabled() == (tag == "aug") and g.pad == CONFIGS[tag]["pad"]
    start, perm = g.next_pairs()
    assert start == 0 and np.array_equal(perm, G[tag + "_perm"])
    if tag == "end":                                   # the next epoch draws the next order from the same stream
        assert np.array_equal(g.next_pairs()[1], G["end_perm2"])
    # the batch split: the recorded batches are the consecutive slices of the order, the last one short
    sizes = [min(16, P - b * 16) for b in range(g.num_batches)]
    if tag == "end":
        sizes = sizes + sizes[:3]
    assert list(G[tag + "_bsizes"]) == sizes[:len(G[tag + "_bsizes"])]


def test_random_state_surface(V, G):
    g = loader(V, G, "a33")
    r = np.random.RandomState(3)
    g.set_random_state(r)
    assert g.random_state() is r
    assert np.array_equal(g.next_pairs()[1], np.array(g.pairs)[np.random.RandomState(3).permutation(len(g.pairs))])
    g = loader(V, G, "end")
    g.state = (2, "kept")                               # endless resume: next_pairs hands back the saved state
    assert g.next_pairs() == (2, "kept")


def test_unshuffled_pairs_are_in_list_order(V, G):
    L = G["len"]
    g = V.GAN_video_ChunkedGenerator(4, None, None, split(G["a33_p2"], L), chunk_length=4, shuffle=False)
    assert np.array_equal(g.next_pairs()[1], np.array(g.pairs))
    # lengths 1, 3, 5: chunks centred on the sequence, [start, end) may reach outside it
    assert g.pairs[:4] == [(0, -1, 3, False), (1, 0, 4, False), (2, -1, 3, False), (2, 3, 7, False)]


def test_bad_arguments_raise_before_any_launch(V, G):
    L = G["len"]
    p3, p2, c = split(G["a33_p3"], L), split(G["a33_p2"], L), cams(G)
    make = V.GAN_video_ChunkedGenerator
    with pytest.raises(ValueError):
        make(16, c, p3[:-1], p2, 1)                    # list lengths differ
    with pytest.raises(ValueError):
        make(16, c[:-1], p3, p2, 1)
    with pytest.raises(ValueError):
        make(16, c, p3, p2, 0)                         # chunk_length < 1
    with pytest.raises(ValueError):
        make(0, c, p3, p2, 1)                          # batch_size < 1
    with pytest.raises(ValueError):
        make(16, c, p3, p2, 1, pad=-1)
    with pytest.raises(ValueError):
        make(16, c, [p[:, :15] for p in p3], p2, 1)    # not 16 joints
    with pytest.raises(ValueError):
        make(16, c, [p[:-1] for p in p3], p2, 1)       # 3D and 2D lengths differ
    with pytest.raises(ValueError):
        make(16, c, p3, p2, 1, augment=True)           # no flip lists
    for bad in (dict(kps_left=[1, 2], kps_right=[3]), dict(kps_left=[1, 2], kps_right=[2, 3]),
                dict(kps_left=[1, 16], kps_right=[2, 3]), dict(joints_left=[4, 4], joints_right=[1, 2])):
        kw = dict(LR)
        kw.update(bad)
        with pytest.raises(ValueError):
            make(16, c, p3, p2, 1, augment=True, **kw)
    with pytest.raises(ValueError):
        make(16, [x[:6] for x in c], p3, p2, 1, augment=True, **LR)   # flip negates camera column 7
    # the data update checks its inputs before it draws or uploads anything
    args = types.SimpleNamespace(batch_size=16, architecture="3,3")
    data = dict(poses_train=p3, poses_train_2d=p2[:-1], actions_train=["a"] * len(p3), cams_train=c)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):
        V.video_mode_dataloader_update(args, data, "cpu")
    data.update(poses_train_2d=p2, cams_train=[x[:8] for x in c])
    with pytest.raises(ValueError):
        V.video_mode_dataloader_update(args, data, "cpu")
    assert np.array_equal(np.random.get_state()[1], state)


def test_clip_gather_argument_errors_without_a_gpu():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    buf = (ctypes.c_float * 256)()
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    mis = ctypes.c_void_p(a.value + 4)
    ident = (ctypes.c_int8 * 16)(*range(16))
    swap = (ctypes.c_int8 * 16)(*([1, 0] + list(range(2, 16))))
    dup = (ctypes.c_int8 * 16)(*([0, 0] + list(range(2, 16))))
    f = L.dhaug_clip_gather
    # (seq3d, seq2d, cams, cam_w, seq_offset, seq_len, records, nrec, frames, pad, causal_shift, perm3d, perm2d, out3d, out2d, out_cam)
    assert f(a, a, a, 16, a, a, a, 0, 9, 4, 0, ident, swap, a, a, a, None) == 0        # empty batch: nothing to do
    assert f(a, a, a, 16, a, a, a, 2, 9, 4, 0, dup, swap, a, a, a, None) == -1         # not a permutation
    assert f(a, a, a, 16, a, a, a, 2, 0, 4, 0, None, None, a, a, a, None) == -1        # frames < 1
    assert f(a, a, a, 16, a, a, a, 2, 9, -1, 0, None, None, a, a, a, None) == -1       # pad < 0
    assert f(a, a, a, 16, a, a, a, 2, 9, 4, 0, None, None, None, a, a, None) == -1     # 3D input without 3D output
    assert f(a, a, None, 16, a, a, a, 2, 9, 4, 0, None, None, a, a, a, None) == -1     # camera output without cameras
    assert f(a, a, a, 0, a, a, a, 2, 9, 4, 0, None, None, a, a, a, None) == -1         # cam_w < 1
    assert f(a, None, a, 16, a, a, a, 2, 9, 4, 0, None, None, a, a, a, None) == -1     # null 2D
    assert f(a, a, a, 16, a, a, mis, 2, 9, 4, 0, None, None, a, a, a, None) == -2      # misaligned records
    assert f(a, mis, a, 16, a, a, a, 2, 9, 4, 0, None, None, a, a, a, None) == -2      # misaligned 2D
    assert f(a, a, a, 16, a, a, a, 1 << 27, 243, 121, 0, None, None, a, a, a, None) == -3   # 2^31 / 12 output rows
