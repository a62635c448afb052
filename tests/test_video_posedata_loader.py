"""CPU checks of the posenet data loaders' host side (ChunkedGenerator / UnchunkedGenerator, no GPU needed): the pair list, the
shuffle order, the batch split and the endless resume equal the reference's (tests/golden/video_posedata.npz, recorded from the
reference's own classes), bad arguments raise at construction, and the two new entry points check their arguments before they
launch anything."""
import ctypes
import os
import sys

import numpy as np
import pytest

import video_posedata_util as U

ROOT = U.ROOT


@pytest.fixture(scope="module")
def V():
    sys.path.insert(0, ROOT)
    from dhaug_amd.models_Fk_GAN import video_mode_operate
    return video_mode_operate


@pytest.fixture(scope="module")
def G():
    return U.load("video_data.npz")


@pytest.fixture(scope="module")
def P():
    return U.load("video_posedata.npz")


@pytest.mark.parametrize("tag", sorted(U.CHUNKED))
def test_pairs_order_and_split_match_the_reference(V, G, P, tag):
    B, kw = U.CHUNKED[tag]
    g = U.chunked(V, G, tag)
    assert np.array_equal(np.array(g.pairs, dtype=np.int64), P[tag + "_pairs"])
    assert all(type(p[3]) is bool for p in g.pairs)
    n = len(g.pairs)
    assert g.num_batches == (n + B - 1) // B and g.num_frames() == g.num_batches * B and g.batch_size == B
    assert g.augment_enabled() == bool(kw.get("augment")) and g.pad == kw["pad"] and g.causal_shift == kw.get("causal_shift", 0)
    start, order = g.next_pairs()
    assert start == 0 and order.dtype == np.int64 and np.array_equal(order, P[tag + "_perm"])
    if kw.get("shuffle", True):
        second = g.next_pairs()[1]                       # the next epoch draws the next order from the same stream
        assert not np.array_equal(second, order)
        if tag == "end":
            assert np.array_equal(second, P["end_perm2"])
    else:
        assert np.array_equal(order, P[tag + "_pairs"]) and np.array_equal(g.next_pairs()[1], order)
    sizes = [min(B, n - b * B) for b in range(g.num_batches)]
    if tag == "end":
        sizes = sizes + sizes[:3]
    assert list(P[tag + "_bsizes"]) == sizes
    if tag == "c333":
        assert sizes[-1] == 1                            # the batch at which the training loop stops


def test_random_state_and_resume_surface(V, G):
    g = U.chunked(V, G, "c33")
    r = np.random.RandomState(3)
    g.set_random_state(r)
    assert g.random_state() is r
    assert np.array_equal(g.next_pairs()[1], np.array(g.pairs)[np.random.RandomState(3).permutation(len(g.pairs))])
    g = U.chunked(V, G, "end")
    assert g.endless and g.state is None
    g.state = (2, "kept")                                # endless resume: next_pairs hands back the saved state
    assert g.next_pairs() == (2, "kept")


def test_windows_of_the_two_members(V, G):
    """the 3D member is the chunk, the 2D member the padded window shifted by causal_shift"""
    g = U.chunked(V, G, "neg")
    assert g._windows() == (3, 0, 7, 0) and g.chunk_length == 3
    g = U.chunked(V, G, "aug")
    assert g._windows() == (4, 0, 8, 3)
    u = U.unchunked(V, G, "u13")
    assert u.num_frames() == int(G["len"].sum()) and not u.augment_enabled()
    u.set_augment(True)
    assert u.augment_enabled()


def test_bad_arguments_raise_at_construction(V, G):
    c, p3, p2 = U.inputs(G, "c33")
    LR = U.LR
    make = V.ChunkedGenerator
    with pytest.raises(ValueError):
        make(16, c, p3[:-1], p2, 1)                      # list lengths differ
    with pytest.raises(ValueError):
        make(16, c[:-1], p3, p2, 1)
    with pytest.raises(ValueError):
        make(16, c, p3, p2, 0)                           # chunk_length < 1
    with pytest.raises(ValueError):
        make(0, c, p3, p2, 1)                            # batch_size < 1
    with pytest.raises(ValueError):
        make(16, c, p3, p2, 1, pad=-1)
    with pytest.raises(ValueError):
        make(16, c, [p[:, :15] for p in p3], p2, 1)      # not 16 joints
    with pytest.raises(ValueError):
        make(16, c, [p[:-1] for p in p3], p2, 1)         # 3D and 2D lengths differ
    with pytest.raises(ValueError):
        make(16, c, p3, p2, 1, augment=True)             # no flip lists
    with pytest.raises(ValueError):
        make(16, c, p3, p2, 1, augment=True, kps_left=[1, 2], kps_right=[2, 3], joints_left=U.LEFT, joints_right=U.RIGHT)
    with pytest.raises(ValueError):
        make(16, [x[:6] for x in c], p3, p2, 1, augment=True, **LR)   # flip negates camera column 7
    # a 2D window wholly outside its sequence (the reference: np.pad "can't extend empty axis" in the middle of the epoch).
    # Sequence 0 has one frame: chunk [0, 1), pad 2, causal_shift 3 -> frames [-5, 0)
    with pytest.raises(ValueError, match="outside sequence"):
        make(16, c, p3, p2, 1, pad=2, causal_shift=3)
    with pytest.raises(ValueError, match="outside sequence"):
        make(16, c, p3, p2, 1, pad=2, causal_shift=-3)
    make(16, c, p3, p2, 1, pad=2, causal_shift=2)        # [-4, 1) still holds frame 0
    with pytest.raises(ValueError):
        make(16, c, None, p2, 1).next_epoch_pairs()      # no targets to train on

    un = V.UnchunkedGenerator
    with pytest.raises(ValueError):
        un(c, p3, p2, pad=3, causal_shift=4)             # np.pad by a negative width
    with pytest.raises(ValueError):
        un(c, p3, p2, pad=3, causal_shift=-4)
    un(c, p3, p2, pad=3, causal_shift=-3)
    with pytest.raises(ValueError):
        un(c, p3[:-1], p2)
    with pytest.raises(ValueError):
        un(c[:-1], p3, p2)
    with pytest.raises(ValueError):
        un(c, p3, [p[:, :15] for p in p2])
    with pytest.raises(ValueError):
        un(c, p3, p2, pad=-1)
    with pytest.raises(ValueError):
        un(c, p3, p2, augment=True)                      # no flip lists
    with pytest.raises(ValueError):
        un([x[:1] for x in c], p3, p2, augment=True, **LR)
    un([x[:1] for x in c], p3, p2, **LR)                 # one-column cameras are fine without augment (the 3DHP loader)
    with pytest.raises(ValueError):
        un(c, [p[:0] for p in p3], [p[:0] for p in p2])  # empty sequences: np.pad cannot extend them
    with pytest.raises(ValueError):
        un(c, p3, p2).set_augment(True)                  # enabling augment later needs the lists too


def test_new_entry_points_check_arguments_without_a_gpu():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    buf = (ctypes.c_float * 256)()
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    mis = ctypes.c_void_p(a.value + 4)
    N = None
    ident = (ctypes.c_int8 * 16)(*range(16))
    swap = (ctypes.c_int8 * 16)(*([1, 0] + list(range(2, 16))))
    dup = (ctypes.c_int8 * 16)(*([0, 0] + list(range(2, 16))))
    big = (ctypes.c_int8 * 16)(*([16] + list(range(1, 16))))

    f = L.dhaug_clip_gather_windows
    # (seq3d, seq2d, cams, cam_w, seq_offset, seq_len, records, nrec, frames3, shift3, frames2, shift2, perm3d, perm2d,
    #  out3d, out2d, out_cam, stream)
    assert f(a, a, a, 16, a, a, a, 0, 1, 0, 9, 4, ident, swap, a, a, a, N) == 0          # empty batch: nothing launched
    assert f(N, a, N, 0, a, a, a, 0, 1, 0, 9, 4, N, N, N, a, N, N) == 0
    assert f(a, a, a, 16, a, a, a, -1, 1, 0, 9, 4, N, N, a, a, a, N) == -1               # negative count
    assert f(a, a, a, 16, a, a, a, 2, 0, 0, 9, 4, N, N, a, a, a, N) == -1                # frames3 < 1
    assert f(a, a, a, 16, a, a, a, 2, 1, 0, 0, 4, N, N, a, a, a, N) == -1                # frames2 < 1
    assert f(a, a, a, 16, a, a, a, 2, 1, 0, 9, 4, dup, N, a, a, a, N) == -1              # not a permutation
    assert f(a, a, a, 16, a, a, a, 2, 1, 0, 9, 4, N, big, a, a, a, N) == -1
    assert f(a, a, a, 16, a, a, a, 2, 1, 0, 9, 4, N, N, N, a, a, N) == -1                # 3D input without 3D output
    assert f(N, a, a, 16, a, a, a, 2, 1, 0, 9, 4, N, N, a, a, a, N) == -1                # 3D output without 3D input
    assert f(a, a, N, 16, a, a, a, 2, 1, 0, 9, 4, N, N, a, a, a, N) == -1                # camera output without cameras
    assert f(a, a, a, 0, a, a, a, 2, 1, 0, 9, 4, N, N, a, a, a, N) == -1                 # cam_w < 1
    assert f(a, N, a, 16, a, a, a, 2, 1, 0, 9, 4, N, N, a, a, a, N) == -1                # null 2D
    assert f(a, a, a, 16, a, a, N, 2, 1, 0, 9, 4, N, N, a, a, a, N) == -1                # null records
    assert f(a, a, a, 16, a, a, mis, 2, 1, 0, 9, 4, N, N, a, a, a, N) == -2              # misaligned records
    assert f(a, mis, a, 16, a, a, a, 2, 1, 0, 9, 4, N, N, a, a, a, N) == -2              # misaligned 2D
    assert f(a, a, a, 16, a, a, a, 2, 1, 0, 9, 4, N, N, mis, a, a, N) == -2              # misaligned 3D output
    assert f(a, a, a, 16, a, a, a, 1 << 27, 1, 0, 243, 121, N, N, a, a, a, N) == -3      # 2^31 / 12 rows of 2D
    assert f(a, a, a, 16, a, a, a, 1 << 27, 243, 0, 1, 0, N, N, a, a, a, N) == -3        # ... of 3D
    assert f(a, a, a, 16, a, a, a, 2, 1, 1 << 30, 9, 4, N, N, a, a, a, N) == -3          # shift out of range

    f = L.dhaug_clip_pair_batch
    # (seq3d, seq2d, seq_offset, seq_len, records, nrec, frames3, shift3, frames2, shift2, perm3d, perm2d, flip, playback,
    #  tgt, inp, tgt_flip, inp_flip, inp_back, inp_flip_back, stream)
    assert f(a, a, a, a, a, 0, 1, 0, 9, 4, ident, swap, 1, 1, a, a, a, a, a, a, N) == 0  # empty batch: nothing launched
    assert f(a, a, a, a, a, -1, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1       # negative count
    assert f(a, a, a, a, a, 2, 0, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1        # frames3 < 1
    assert f(a, a, a, a, a, 2, 1, 0, 0, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1        # frames2 < 1
    assert f(a, a, a, a, a, 2, 1, 0, 9, 4, N, N, 0, 0, N, N, N, N, N, N, N) == -1        # no output at all
    assert f(a, a, a, a, a, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, a, N, N, N, N) == -1        # tgt_flip without flip
    assert f(a, a, a, a, a, 2, 1, 0, 9, 4, N, N, 1, 0, a, a, a, a, a, N, N) == -1        # inp_back without playback
    assert f(a, a, a, a, a, 2, 1, 0, 9, 4, N, N, 0, 1, a, a, N, N, a, a, N) == -1        # inp_flip_back without flip
    assert f(N, a, a, a, a, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1        # tgt asked for, seq3d NULL
    assert f(a, N, a, a, a, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1        # inp asked for, seq2d NULL
    assert f(a, a, a, a, a, 2, 1, 0, 9, 4, dup, N, 0, 0, a, a, N, N, N, N, N) == -1      # not a permutation
    assert f(a, a, N, a, a, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1        # null table
    assert f(a, a, a, N, a, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1
    assert f(a, a, a, a, N, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -1
    assert f(a, a, a, a, mis, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -2      # misaligned records
    assert f(a, a, mis, a, a, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -2      # misaligned offsets (8 bytes)
    assert f(mis, a, a, a, a, 2, 1, 0, 9, 4, N, N, 0, 0, a, a, N, N, N, N, N) == -2      # misaligned sequences
    assert f(a, a, a, a, a, 2, 1, 0, 9, 4, N, N, 1, 1, a, a, a, a, a, mis, N) == -2      # misaligned output
    assert f(a, a, a, a, a, 1 << 27, 1, 0, 243, 121, N, N, 0, 0, a, a, N, N, N, N, N) == -3   # 2^31 / 12 rows
    assert f(a, a, a, a, a, 2, 1, 0, 9, -(1 << 30), N, N, 0, 0, a, a, N, N, N, N, N) == -3    # shift out of range
