"""The pieces of R/models_Fk_GAN/video_mode_operate.py that the video GAN epoch reads: the receptive field, and the
real-clip loader of the multi-frame mode (GAN_video_ChunkedGenerator :35-192, video_mode_random_bl_aug :879-896,
video_mode_dataloader_update :898-968) kept on the device.

The loader's sequences sit concatenated in device memory; every batch is one dhaug_clip_gather launch over a slice of the
epoch's permuted record table (uploaded once per epoch), so there is no host work per clip and no host <-> device copy per
batch.  Batches are device fp32 tensors; they equal the reference's float64 numpy batches cast to fp32 bit for bit (the
gather only copies, negates and permutes).  ChunkedGenerator (:193-347) and UnchunkedGenerator (:350-406), the loaders of the
posenet's real clips and of its evaluation sets, stand on the same plumbing with a window of their own for the 3D target
(dhaug_clip_gather_windows, dhaug_clip_pair_batch).  Also here: the posenet evaluation and training loops of the video mode
(video_mode_evaluate, video_mode_train_posenet, GAN_dataSet_video_mode_train_posenet), see function_aug/model_pos_eval.py and
function_aug/model_pos_train.py."""
import numpy as np
import torch

from .. import ops
from ..function_aug.dataloader_update import BL_TEMPLATES


def video_receptive_field(filter_widths):
    """frames per sample = product of the temporal filter widths (R/models_Fk_GAN/video_mode_operate.py:411-415)."""
    frames = 1
    for w in filter_widths:
        frames *= w
    return frames


def frames_from_args(args):
    if getattr(args, "single_or_multi_train_mode", "single") == "multi":
        return video_receptive_field([int(x) for x in args.architecture.split(",")])
    return 1


# left / right joints of the 16-joint H36M skeleton, for the 2D keypoints and the 3D joints alike (:940-943)
JOINTS_LEFT = [4, 5, 6, 10, 11, 12]
JOINTS_RIGHT = [1, 2, 3, 13, 14, 15]


def _int(v, name, lo):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, lo, v))
    return int(v)


def _flip_perm(left, right, name):
    """joint permutation of a flip: out[left] = in[right], out[right] = in[left]; the lists must be a disjoint pair"""
    if left is None or right is None:
        raise ValueError("augment=True needs %s_left and %s_right" % (name, name))
    left, right = [int(j) for j in left], [int(j) for j in right]
    both = left + right
    if len(left) != len(right) or len(set(both)) != len(both) or any(j < 0 or j >= 16 for j in both):
        raise ValueError("%s_left / %s_right must be two disjoint lists of equal length over joints 0..15: %r %r"
                         % (name, name, left, right))
    perm = list(range(16))
    for a, b in zip(left, right):
        perm[a], perm[b] = b, a
    return perm


class _ResidentSequences:
    """what the loaders below share: the reference's lists of per-sequence arrays checked and concatenated once on the host,
    uploaded to the current device at the first epoch, with each sequence's first row and length beside them"""

    @staticmethod
    def _check_lists(cameras, poses_3d, poses_2d):
        if poses_2d is None or len(poses_2d) == 0:
            raise ValueError("poses_2d must be a non-empty list of (frames, 16, 2) arrays")
        S = len(poses_2d)
        if poses_3d is not None and len(poses_3d) != S:
            raise ValueError("poses_3d and poses_2d differ in length: %d vs %d" % (len(poses_3d), S))
        if cameras is not None and len(cameras) != S:
            raise ValueError("cameras and poses_2d differ in length: %d vs %d" % (len(cameras), S))
        p2 = [np.asarray(p) for p in poses_2d]
        lengths = np.array([p.shape[0] for p in p2], dtype=np.int64)
        for i, p in enumerate(p2):
            if p.shape[1:] != (16, 2):
                raise ValueError("poses_2d[%d] has shape %s, expected (frames, 16, 2)" % (i, p.shape))
        p3 = None
        if poses_3d is not None:
            p3 = [np.asarray(p) for p in poses_3d]
            for i, p in enumerate(p3):
                if p.shape != (lengths[i], 16, 3):
                    raise ValueError("poses_3d[%d] has shape %s, expected (%d, 16, 3)" % (i, p.shape, lengths[i]))
        cam = None
        if cameras is not None:
            cam = [np.asarray(c).reshape(-1) for c in cameras]
            if len({c.shape[0] for c in cam}) != 1:
                raise ValueError("cameras differ in width")
        return lengths, cam, p3, p2

    def _keep_host(self, cam, p3, p2):
        # one concatenation per construction; the upload follows at the first next_epoch()
        cat = lambda xs, w: np.concatenate([x.reshape(-1, 16, w) for x in xs]).astype(np.float32, copy=False)
        self._host = (None if cam is None else np.stack(cam).astype(np.float32, copy=False),
                      None if p3 is None else cat(p3, 3), cat(p2, 2))
        self._dev = None

    @staticmethod
    def _check_device(cams, seq3d, seq2d, lengths):
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        T = int(lengths.sum())
        if (lengths < 0).any() or tuple(seq2d.shape) != (T, 16, 2) or (seq3d is not None and tuple(seq3d.shape) != (T, 16, 3)):
            raise ValueError("device sequences do not match the lengths")
        if cams is not None and (cams.dim() != 2 or cams.shape[0] != lengths.shape[0]):
            raise ValueError("cams must be (sequences, cam_w)")
        return lengths

    def _put(self, cams, seq3d, seq2d):
        dev = seq2d.device
        starts = np.concatenate([[0], np.cumsum(self._lengths)[:-1]]).astype(np.int64)
        self._dev = dict(cams=cams, seq3d=seq3d, seq2d=seq2d,
                         offset=torch.from_numpy(starts).to(dev),
                         length=torch.from_numpy(self._lengths.astype(np.int32)).to(dev))

    def _device_data(self):
        if self._dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
            cams, seq3d, seq2d = self._host
            self._put(up(cams), up(seq3d), up(seq2d))
            self._host = None
        return self._dev


class GAN_video_ChunkedGenerator(_ResidentSequences):
    """Drop-in for GAN_video_ChunkedGenerator (R/models_Fk_GAN/video_mode_operate.py:35-192).

    Same signature, pair list, shuffle stream (np.random.RandomState(random_seed)), batch split and endless / state
    resume as the reference.  Differences: next_epoch() yields (cam, poses_3d, poses_2d) as DEVICE fp32 tensors (None where
    the reference yields None), freshly allocated per batch; next_pairs() returns the pairs as an (P, 4) int64 array also
    without shuffle.  Poses are 16 joints: (frames, 16, 3) and (frames, 16, 2) per sequence, cameras one vector each.  The
    lists are concatenated once here and uploaded to the current device at the first next_epoch()."""

    def __init__(self, batch_size, cameras, poses_3d, poses_2d, chunk_length, pad=0, causal_shift=0, shuffle=True,
                 random_seed=1234, augment=False, kps_left=None, kps_right=None, joints_left=None, joints_right=None,
                 endless=False):
        lengths, cam, p3, p2 = self._check_lists(cameras, poses_3d, poses_2d)
        self._setup(batch_size, lengths, None if cam is None else cam[0].shape[0], p3 is not None, chunk_length, pad,
                    causal_shift, shuffle, random_seed, augment, kps_left, kps_right, joints_left, joints_right, endless)
        self._keep_host(cam, p3, p2)

    @classmethod
    def _from_device(cls, batch_size, cams, seq3d, seq2d, lengths, chunk_length, **kw):
        """the same loader over sequences already concatenated on the device: cams (S, cam_w) or None, seq3d (T,16,3) or
        None, seq2d (T,16,2) fp32 device tensors, lengths (S,) host integers summing to T; keyword arguments as __init__"""
        self = cls.__new__(cls)
        lengths = cls._check_device(cams, seq3d, seq2d, lengths)
        self._setup(batch_size, lengths, None if cams is None else cams.shape[1], seq3d is not None, chunk_length, **kw)
        self._host = None
        self._put(cams, seq3d, seq2d)
        return self

    def _setup(self, batch_size, lengths, cam_w, has3d, chunk_length, pad=0, causal_shift=0, shuffle=True,
               random_seed=1234, augment=False, kps_left=None, kps_right=None, joints_left=None, joints_right=None,
               endless=False):
        batch_size = _int(batch_size, "batch_size", 1)
        cl = _int(chunk_length, "chunk_length", 1)
        pad = _int(pad, "pad", 0)
        causal_shift = _int(causal_shift, "causal_shift", -(1 << 29))
        if pad >= (1 << 29) or causal_shift >= (1 << 29):
            raise ValueError("pad / causal_shift out of range")
        if int(lengths.sum()) >= (1 << 31) - 2 * cl:
            raise ValueError("the sequences hold %d frames; at most 2^31 are supported" % int(lengths.sum()))
        self._perm2d = self._perm3d = None
        if augment:
            self._perm2d = _flip_perm(kps_left, kps_right, "kps")
            if has3d:
                self._perm3d = _flip_perm(joints_left, joints_right, "joints")
            if cam_w is not None and cam_w < 8:
                raise ValueError("augment flips camera columns 2 and 7: cameras need >= 8 columns, got %d" % cam_w)
        # the pair list: per sequence its chunks [start, end), centred on the sequence, then (augment) the same flipped
        n = (lengths + cl - 1) // cl
        off = (n * cl - lengths) // 2
        reps = n * (2 if augment else 1)
        P = int(reps.sum())
        seq = np.repeat(np.arange(len(lengths), dtype=np.int64), reps)
        m = np.arange(P, dtype=np.int64) - np.repeat(np.cumsum(reps) - reps, reps)
        nn = np.repeat(n, reps)
        start = (m % np.maximum(nn, 1)) * cl - np.repeat(off, reps)
        self._pair_arr = np.stack([seq, start, start + cl, (m >= nn).astype(np.int64)], axis=1).reshape(P, 4)
        self._pairs = None
        self._lengths = lengths
        self._cam_w, self._has3d = cam_w, has3d
        self.frames = cl + 2 * pad
        self.num_batches = (P + batch_size - 1) // batch_size
        self.batch_size = batch_size
        self.random = np.random.RandomState(random_seed)
        self.shuffle = shuffle
        self.pad = pad
        self.causal_shift = causal_shift
        self.endless = endless
        self.state = None
        self.augment = augment
        self.kps_left, self.kps_right, self.joints_left, self.joints_right = kps_left, kps_right, joints_left, joints_right
        self._records = (None, None)

    @property
    def pairs(self):
        """the reference's pair list: (seq_idx, start_frame, end_frame, flip) tuples"""
        if self._pairs is None:
            self._pairs = [(int(s), int(a), int(b), bool(f)) for s, a, b, f in self._pair_arr]
        return self._pairs

    def num_frames(self):
        return self.num_batches * self.batch_size

    def random_state(self):
        return self.random

    def set_random_state(self, random):
        self.random = random

    def augment_enabled(self):
        return self.augment

    def next_pairs(self):
        if self.state is None:
            # RandomState.permutation(P) draws the order the reference's permutation(pairs) does
            pairs = self._pair_arr[self.random.permutation(len(self._pair_arr))] if self.shuffle else self._pair_arr
            return 0, pairs
        return self.state

    def _device_records(self, pairs, dev):
        """pairs (P, 4) -> int32 device table, uploaded once per epoch (kept while the same array comes back on resume)"""
        if self._records[0] is not pairs:
            self._records = (pairs, torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(dev))
        return self._records[1]

    def _batches(self, launch):
        """the epoch loop: launch(device data, this batch's slice of the record table) per batch, with the reference's endless /
        state bookkeeping"""
        d = self._device_data()
        B = self.batch_size
        while True:
            start_idx, pairs = self.next_pairs()
            rec = self._device_records(pairs, d["seq2d"].device)
            for b in range(start_idx, self.num_batches):
                out = launch(d, rec[b * B:(b + 1) * B])
                if self.endless:
                    self.state = (b + 1, pairs)
                yield out
            if not self.endless:
                return
            self.state = None

    def next_epoch(self):
        return self._batches(lambda d, rec: ops.clip_gather(d["seq3d"], d["seq2d"], d["cams"], d["offset"], d["length"], rec,
                                                            self.frames, self.pad, self.causal_shift, self._perm3d,
                                                            self._perm2d))


class ChunkedGenerator(GAN_video_ChunkedGenerator):
    """Drop-in for ChunkedGenerator (R/models_Fk_GAN/video_mode_operate.py:193-347), the loader of the posenet's real clips
    (data_dict['train_det2d3d_loader']) and, with shuffle=False, of the non-temporal posenets' validation sets (:476-511).

    It differs from GAN_video_ChunkedGenerator in its 3D member: batch_3d (n, chunk_length, 16, 3) holds the frames of the
    chunk itself, without pad and causal_shift; batch_2d (n, chunk_length + 2 pad, 16, 2) is the padded, shifted window.  Same
    signature, pair list, RandomState(random_seed).permutation stream, batch split and endless / state resume as the reference;
    the differences are those of GAN_video_ChunkedGenerator (device fp32 batches, one dhaug_clip_gather_windows launch each,
    next_pairs() an int64 array), and a 2D window that lies wholly outside its sequence (a large |causal_shift|: the
    reference's np.pad raises "can't extend empty axis" in the middle of an epoch) is a ValueError here, at construction.
    next_epoch_pairs(flip, playback) yields what one iteration of video_mode_train_posenet reads, ops.pair_batch's dict, from
    one dhaug_clip_pair_batch launch per batch."""

    def _setup(self, batch_size, lengths, cam_w, has3d, chunk_length, pad=0, causal_shift=0, *args, **kw):
        super()._setup(batch_size, lengths, cam_w, has3d, chunk_length, pad, causal_shift, *args, **kw)
        self.chunk_length = self.frames - 2 * self.pad
        seq, start, end = self._pair_arr[:, 0], self._pair_arr[:, 1], self._pair_arr[:, 2]
        low = np.maximum(start - self.pad - self.causal_shift, 0)
        high = np.minimum(end + self.pad - self.causal_shift, lengths[seq])
        if (low >= high).any():
            i = int(np.argmax(low >= high))
            raise ValueError("pad %d, causal_shift %d: the 2D window of chunk [%d, %d) lies outside sequence %d of %d frames"
                             % (self.pad, self.causal_shift, start[i], end[i], seq[i], lengths[seq[i]]))

    def _windows(self):
        return self.chunk_length, 0, self.frames, self.pad + self.causal_shift

    def next_epoch(self):
        return self._batches(lambda d, rec: ops.clip_gather_windows(d["seq3d"], d["seq2d"], d["cams"], d["offset"], d["length"],
                                                                    rec, *self._windows(), self._perm3d, self._perm2d))

    def next_epoch_pairs(self, flip=False, playback=False):
        """the epoch next_epoch() yields, each batch as ops.pair_batch(batch_3d, batch_2d, flip=flip, playback=playback) would
        make it, bit for bit, without the gathered batch in between"""
        if not self._has3d:
            raise ValueError("next_epoch_pairs needs poses_3d: the training targets")
        return self._batches(lambda d, rec: ops.clip_pair_batch(d["seq3d"], d["seq2d"], d["offset"], d["length"], rec,
                                                                *self._windows(), self._perm3d, self._perm2d, flip=flip,
                                                                playback=playback))


class UnchunkedGenerator(_ResidentSequences):
    """Drop-in for UnchunkedGenerator (R/models_Fk_GAN/video_mode_operate.py:350-406), the evaluation loader of the temporal
    posenets (data_dict['H36M_test'], data_dict['mpi3d_loader']): next_epoch() yields one sequence per batch,
    (cam (m, cam_w), batch_3d (m, T, 16, 3), batch_2d (m, T + 2 pad, 16, 2)) with m = 2 under augment (row 1 the flipped copy),
    else 1; None where the reference yields None.  Batches are fresh device fp32 tensors equal to the reference's float64
    batches cast to fp32 bit for bit: the sequences are uploaded once, each batch is one dhaug_clip_gather_windows launch over the
    records (seq, 0, T, 0[, 1]).  pad < |causal_shift| (np.pad's negative width) and an empty sequence are ValueErrors here, at
    construction, and so are the flip lists and cameras augment cannot work with."""

    def __init__(self, cameras, poses_3d, poses_2d, pad=0, causal_shift=0, augment=False, kps_left=None, kps_right=None,
                 joints_left=None, joints_right=None):
        lengths, cam, p3, p2 = self._check_lists(cameras, poses_3d, poses_2d)
        self._setup(lengths, None if cam is None else cam[0].shape[0], p3 is not None, pad, causal_shift, augment, kps_left,
                    kps_right, joints_left, joints_right)
        self._keep_host(cam, p3, p2)

    @classmethod
    def _from_device(cls, cams, seq3d, seq2d, lengths, **kw):
        """the same loader over sequences already concatenated on the device (see GAN_video_ChunkedGenerator._from_device)"""
        self = cls.__new__(cls)
        lengths = cls._check_device(cams, seq3d, seq2d, lengths)
        self._setup(lengths, None if cams is None else cams.shape[1], seq3d is not None, **kw)
        self._host = None
        self._put(cams, seq3d, seq2d)
        return self

    def _setup(self, lengths, cam_w, has3d, pad=0, causal_shift=0, augment=False, kps_left=None, kps_right=None,
               joints_left=None, joints_right=None):
        pad = _int(pad, "pad", 0)
        causal_shift = _int(causal_shift, "causal_shift", -(1 << 29))
        if pad >= (1 << 29):
            raise ValueError("pad out of range")
        if pad < abs(causal_shift):
            raise ValueError("pad %d < |causal_shift| %d: the 2D sequence would be padded by a negative width" % (pad, causal_shift))
        if (lengths < 1).any():
            raise ValueError("sequence %d is empty" % int(np.argmax(lengths < 1)))
        if int(lengths.max()) + 2 * pad >= (1 << 31) // 12 // 2 or int(lengths.sum()) >= (1 << 31) - 1:
            raise ValueError("sequences too long: at most 2^31 / 24 frames per padded sequence are supported")
        self._lengths, self._cam_w, self._has3d = lengths, cam_w, has3d
        self.pad, self.causal_shift = pad, causal_shift
        self.kps_left, self.kps_right, self.joints_left, self.joints_right = kps_left, kps_right, joints_left, joints_right
        self._records = None
        self.set_augment(augment)

    def num_frames(self):
        return int(self._lengths.sum())

    def augment_enabled(self):
        return self.augment

    def set_augment(self, augment):
        self._perm2d = self._perm3d = None
        if augment:
            self._perm2d = _flip_perm(self.kps_left, self.kps_right, "kps")
            if self._has3d:
                self._perm3d = _flip_perm(self.joints_left, self.joints_right, "joints")
            if self._cam_w is not None and self._cam_w < 8:
                raise ValueError("augment flips camera columns 2 and 7: cameras need >= 8 columns, got %d" % self._cam_w)
        self.augment = augment

    def next_epoch(self):
        d = self._device_data()
        if self._records is None:
            # rows 2s and 2s + 1: sequence s as it is and flipped; uploaded once
            S = len(self._lengths)
            rec = np.zeros((2 * S, 4), dtype=np.int32)
            rec[:, 0] = np.repeat(np.arange(S), 2)
            rec[:, 2] = np.repeat(self._lengths, 2)
            rec[1::2, 3] = 1
            self._records = torch.from_numpy(rec).to(d["seq2d"].device)
        shift = self.pad + self.causal_shift
        for s, T in enumerate(self._lengths):
            T = int(T)
            yield ops.clip_gather_windows(d["seq3d"], d["seq2d"], d["cams"], d["offset"], d["length"],
                                          self._records[2 * s:2 * s + (2 if self.augment else 1)], T, 0, T + 2 * self.pad, shift,
                                          self._perm3d, self._perm2d)


def video_mode_random_bl_aug(x, template_idx=None):
    """Drop-in for video_mode_random_bl_aug (:879-896): x (N,16,3), one sequence -> every frame's bones keep their directions
    and take the lengths of ONE template (drawn with np.random.choice(5, 1) as at :888, or given)."""
    if template_idx is None:
        template_idx = np.random.choice(BL_TEMPLATES.shape[0], 1)
    k = int(np.asarray(template_idx).reshape(-1)[0])
    x = x.reshape(-1, 16, 3)
    lens = torch.as_tensor(BL_TEMPLATES[k], device=x.device).expand(x.shape[0], 15)
    return ops.bone_length_swap(x, lens)


def video_mode_dataloader_update(args, data_dict, device):
    """Drop-in for video_mode_dataloader_update (:898-968): bone-length swap of every training sequence (one template per
    sequence) and re-projection with the sequence's camera, then data_dict['target_GAN_loader'] over the results.

    The whole epoch is one upload of the raw sequences, one dhaug_bone_length_swap and one dhaug_project_to_2d launch over
    all frames (per-row template and camera rows); nothing is copied back.  The template draws stay on the host, one
    np.random.choice per sequence in sequence order, so the global numpy stream advances as in the reference.  As in the
    reference, the loader is built with the default seed 1234 every epoch, so every epoch sees the same clip order."""
    poses, cams = data_dict['poses_train'], data_dict['cams_train']
    S = len(poses)
    for key in ('poses_train_2d', 'actions_train', 'cams_train'):
        if len(data_dict[key]) != S:
            raise ValueError("data_dict['%s'] has %d entries, poses_train %d" % (key, len(data_dict[key]), S))
    if S == 0:
        raise ValueError("data_dict['poses_train'] is empty")
    lengths = np.array([np.shape(p)[0] for p in poses], dtype=np.int64)
    for i, p in enumerate(poses):
        if np.shape(p)[1:] != (16, 3):
            raise ValueError("poses_train[%d] has shape %s, expected (frames, 16, 3)" % (i, np.shape(p)))
    cam = [np.asarray(c, dtype=np.float32).reshape(-1) for c in cams]
    if len({c.shape[0] for c in cam}) != 1 or cam[0].shape[0] < 9:
        raise ValueError("cams_train must be vectors of one width >= 9")
    R = video_receptive_field([int(w) for w in args.architecture.split(',')])
    tmpl = np.array([np.random.choice(BL_TEMPLATES.shape[0], 1)[0] for _ in range(S)], dtype=np.int64)

    T = int(lengths.sum())
    x = torch.from_numpy(np.concatenate([np.asarray(p, dtype=np.float32) for p in poses])).to(device)
    cam = torch.from_numpy(np.stack(cam)).to(device)
    seq_of_row = torch.repeat_interleave(torch.arange(S, device=device), torch.from_numpy(lengths).to(device),
                                         output_size=T)
    row_tmpl = torch.from_numpy(tmpl).to(device)[seq_of_row]
    p3 = ops.bone_length_swap(x, torch.as_tensor(BL_TEMPLATES, device=device)[row_tmpl])
    p2 = ops.project_to_2d(p3, cam[:, :9][seq_of_row])
    data_dict['target_GAN_loader'] = GAN_video_ChunkedGenerator._from_device(
        args.batch_size // 1, cam, p3, p2, lengths, chunk_length=1, pad=(R - 1) // 2, causal_shift=0, shuffle=True,
        augment=False, kps_left=JOINTS_LEFT, kps_right=JOINTS_RIGHT, joints_left=JOINTS_LEFT, joints_right=JOINTS_RIGHT)
    return


def _upload_batch(b, device):
    """a next_epoch() batch -> device fp32: numpy (the reference's ChunkedGenerator) through pinned memory, tensors as they are"""
    if torch.is_tensor(b):
        return b.to(device=device, dtype=torch.float32, non_blocking=True)
    t = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32))
    return t.pin_memory().to(device, non_blocking=True)


def video_mode_evaluate(args, data_loader, model_pos_eval, device, summary=None,
                        writer=None, key='', tag='', flipaug='', get_pck_auc=False):
    """Drop-in for video_mode_evaluate (R/models_Fk_GAN/video_mode_operate.py:769-859): the reference's reshapes, posenet calls
    and flip (dhaug_center_flip per frame); the metrics are summed on the device and read once, at the end (see
    function_aug/model_pos_eval.py).  Returns (p1 mm, p2 mm, pck %, auc %).

    data_loader.next_epoch() may yield host numpy batches (the reference's generators) or device tensors: this package's
    UnchunkedGenerator and ChunkedGenerator(shuffle=False) are taken as they come, with no copy and no host read per batch."""
    from ..function_aug.model_pos_eval import finish, flip_pose, write_scalars
    from ..utils.loss import PoseMetricsAccumulator

    receptive_field = video_receptive_field([int(x) for x in args.architecture.split(',')])
    model_pos_eval.eval()
    acc = PoseMetricsAccumulator(device, center=True)
    for _cam, batch_3d, batch_2d in data_loader.next_epoch():
        if tuple(batch_3d.shape[-2:]) != (16, 3) or tuple(batch_2d.shape[-2:]) != (16, 2):
            raise ValueError("video_mode_evaluate: 16-joint batches expected, got %s and %s"
                             % (tuple(batch_3d.shape), tuple(batch_2d.shape)))
        targets_3d, inputs_2d = _upload_batch(batch_3d, device), _upload_batch(batch_2d, device)
        if args.posenet_name != 'mulit_farme_videopose':
            inputs_2d = inputs_2d.view(-1, receptive_field, 16, 2)
            targets_3d = targets_3d.view(-1, 1, 16, 3)
        with torch.no_grad():
            if flipaug:
                outputs_3d_flip = flip_pose(model_pos_eval(flip_pose(inputs_2d)))
                outputs_3d = model_pos_eval(inputs_2d)
                outputs_3d = (outputs_3d + outputs_3d_flip) / 2.0
            else:
                outputs_3d = model_pos_eval(inputs_2d)
        acc.add(outputs_3d, targets_3d)
    p1, p2, pck, auc = finish(acc, get_pck_auc, key)
    write_scalars(writer, summary, key, tag, flipaug, p1, p2, pck, auc)
    return p1, p2, pck, auc


def video_mode_evaluate_posenet(args, data_dict, model_pos, model_pos_eval,
                                device, summary, writer, tag, get_pck_auc=False):
    """Drop-in for video_mode_evaluate_posenet (:862-876): H36M without and 3DHP with the test-time flip"""
    with torch.no_grad():
        model_pos_eval.load_state_dict(model_pos.state_dict())
        h36m_p1, h36m_p2, _, _ = video_mode_evaluate(args, data_dict['H36M_test'], model_pos_eval, device, summary, writer,
                                                     key='H36M_test', tag=tag, flipaug='')
        dhp_p1, dhp_p2, PCK, AUC = video_mode_evaluate(args, data_dict['mpi3d_loader'], model_pos_eval, device, summary,
                                                       writer, key='mpi3d_loader', tag=tag, flipaug='_flip',
                                                       get_pck_auc=get_pck_auc)
    return h36m_p1, h36m_p2, dhp_p1, dhp_p2, PCK, AUC


def _video_train_epoch(fn, title, batches, model_pos, optimizer, criterion, device, args, single_frame_targets):
    """the epoch both video training loops share: per batch up to four steps in the reference's order -- plain, playback, flip,
    flip + playback (R/models_Fk_GAN/video_mode_operate.py:566-629, :686-749)"""
    from ..function_aug.model_pos_train import StepRunner, graph_requested, set_grad, summary_line
    torch.set_grad_enabled(True)
    set_grad([model_pos], True)
    model_pos.train()
    run = StepRunner(model_pos, optimizer, criterion, device, graph=graph_requested(args))
    flip, playback = bool(args.flip_pos_model_input), args.GAN_video_playback_input == True  # noqa: E712 (the reference's test)
    for b in batches(flip, playback):
        num_poses = b["inp"].shape[0]
        if num_poses == 1:
            break
        tgt, tgt_flip = b["tgt"], b.get("tgt_flip")
        if single_frame_targets:                                   # batch_3d.contiguous().view(-1, 1, 16, 3) (:679)
            tgt = tgt.view(-1, 1, 16, 3)
            tgt_flip = None if tgt_flip is None else tgt_flip.view(-1, 1, 16, 3)
        run.step(b["inp"], tgt, "loss", num_poses)
        if playback:
            run.step(b["inp_back"], tgt, "back_loss", num_poses)
        if flip:
            # the reference updates its flip meter with the plain step's loss (:614, :734): StepRunner.finish copies the plain meter
            run.step(b["inp_flip"], tgt_flip, None, num_poses)
            if playback:
                run.step(b["inp_flip_back"], tgt_flip, "back_flip_loss", num_poses)
    fn.last_meters = run.finish(flip)
    fn.last_trace = run.trace_tensor()
    summary_line(title, fn.last_meters)


def video_mode_train_posenet(model_pos, data_loader, optimizer, criterion, device, args):
    """Drop-in for video_mode_train_posenet (R/models_Fk_GAN/video_mode_operate.py:532-648) over data_loader.next_epoch() yielding
    (cam, batch_3d (n,F3,16,3), batch_2d (n,F2,16,2)): device tensors (this package's GAN_video_ChunkedGenerator) or host numpy
    batches (the reference's generators).  A loader with next_epoch_pairs(flip, playback) (this package's ChunkedGenerator) is asked
    for the iteration's tensors directly: one dhaug_clip_pair_batch launch per batch from the resident sequences, the same bits.  See function_aug/model_pos_train.py for what runs where; returns None, the epoch's
    averages are on video_mode_train_posenet.last_meters."""
    def batches(flip, playback):
        if hasattr(data_loader, "next_epoch_pairs"):    # this package's ChunkedGenerator: one launch per batch, no host batch
            # (a batch of one pose is yielded as it is: _video_train_epoch stops there, as the reference's loop does)
            yield from data_loader.next_epoch_pairs(flip, playback)
            return
        for _cam, batch_3d, batch_2d in data_loader.next_epoch():
            if batch_3d.shape[0] == 1:                  # the reference's loop stops at a batch of one pose
                return
            yield ops.pair_batch(_upload_batch(batch_3d, device), _upload_batch(batch_2d, device), flip=flip, playback=playback)

    _video_train_epoch(video_mode_train_posenet, "Train posenet (video)", batches, model_pos, optimizer, criterion, device, args,
                       False)
    return


def GAN_dataSet_video_mode_train_posenet(model_pos, data_loader, optimizer, criterion,
                                         device, args):
    """Drop-in for GAN_dataSet_video_mode_train_posenet (:652-765) over a loader of (cam, batch_3d, batch_2d) batches, or over the
    device-resident product of the video GAN epoch (FakePairBuffer / TensorLoader: one permutation per epoch, one launch per
    batch).  The 3D rows are viewed as (-1, 1, 16, 3) as at :679."""
    from ..function_aug.model_pos_train import pair_batches

    def batches(flip, playback):
        return pair_batches(data_loader, device, flip, playback, lambda batch: (batch[1], batch[2]))

    _video_train_epoch(GAN_dataSet_video_mode_train_posenet, "Train posenet (GAN clips)", batches, model_pos, optimizer,
                       criterion, device, args, True)
    return


for _f in (video_mode_train_posenet, GAN_dataSet_video_mode_train_posenet):
    _f.last_meters = None
    _f.last_trace = None
