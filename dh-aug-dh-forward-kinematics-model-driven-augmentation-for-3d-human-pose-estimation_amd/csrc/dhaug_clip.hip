// Clip gather of the video GAN's real-data loader (GAN_video_ChunkedGenerator.next_epoch,
// R/models_Fk_GAN/video_mode_operate.py:126-183): one launch writes a whole batch of (frames, 16, C) clips from the
// concatenated device-resident sequences.  Pure data movement -- a copy, a sign flip and a joint permutation -- so the
// output equals the reference's float64 batch cast to fp32 bit for bit.
//
// Work items, one flat index space: the 16-byte quads of the 3D frames (12 per frame), then those of the 2D frames (8 per
// frame), then the camera scalars.  Every store is a 16-byte store of consecutive output addresses (the camera's a 4-byte one);
// an unflipped quad is one 16-byte load of the source frame, a flipped one four scalar loads through the joint permutation.
// A batch is a few MB: latency-bound, one short launch.
//
// dhaug_clip_gather_windows is the same kernel with a window of its own for the 3D and the 2D frames: the posenet loaders
// (ChunkedGenerator :193-347, UnchunkedGenerator :350-406) take the chunk's frames as the 3D target and the padded, shifted
// window as the 2D input.  dhaug_clip_gather is the case of two equal windows.  dhaug_clip_pair_batch goes one step further and
// writes what one posenet training iteration reads (dhaug_pair_batch's outputs) straight from the sequences.
#include "dhaug_common.h"
#include "dhaug_pose_regs.h"

namespace {

struct ClipArgs {
    const float* seq3d;
    const float* seq2d;
    const float* cams;
    const long long* seq_offset;
    const int* seq_len;
    const int4* records;          // (seq, start, end, flip)
    float* out3d;
    float* out2d;
    float* out_cam;
    unsigned long long perm3d;    // joint j <- joint (perm >> 4j) & 15 on flip (a by-value array indexed by a lane value
    unsigned long long perm2d;    // would go to scratch; the packed word stays in SGPRs)
    long long n3;                 // quads of out3d (0 without 3D)
    long long n2;                 // quads of out2d
    long long ncam;               // scalars of out_cam (0 without cameras)
    int frames3, shift3;          // the 3D window: output frame f reads frame start - shift3 + f, clamped to the sequence
    int frames2, shift2;          // the 2D window (dhaug_clip_gather: both windows are (frames, pad + causal_shift))
    int cam_w;
};

// source frame (absolute row of the concatenated sequences) of frame f of a window shifted by `shift` of record r: the slice
// [start - shift, start - shift + frames) with the 'edge' padding of np.pad
__device__ __forceinline__ long long clip_frame(const long long* __restrict__ seq_offset, const int* __restrict__ seq_len,
                                                const int4 r, int shift, int f) {
    const long long last = seq_len[r.x] - 1;
    long long t = (long long)r.y - shift + f;
    t = t < 0 ? 0 : (t > last ? last : t);
    return seq_offset[r.x] + t;
}

// quad q (4 floats) of an output frame of 16 joints x W coordinates
template <int W>
__device__ __forceinline__ void clip_quad(const float* __restrict__ seq, float* __restrict__ out, long long i,
                                          const ClipArgs& a, unsigned long long perm, int frames, int shift) {
    constexpr int QPF = 16 * W / 4;                   // quads per frame: 12 (3D), 8 (2D)
    const int row = (int)(i / QPF), q = (int)(i - (long long)row * QPF);
    const int rec = row / frames, f = row - rec * frames;
    const int4 r = a.records[rec];
    const float* s = seq + clip_frame(a.seq_offset, a.seq_len, r, shift, f) * (16 * W);
    float4 v;
    if (r.w == 0) {
        v = *reinterpret_cast<const float4*>(s + q * 4);
    } else {
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = q * 4 + k, j = c / W, d = c - j * W;
            const int src = (int)((perm >> (4 * j)) & 15u);
            const float x = s[src * W + d];
            e[k] = d == 0 ? -x : x;                   // x -> -x, then joint j <- joint perm[j]
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
    }
    *reinterpret_cast<float4*>(out + i * 4) = v;
}

__global__ __launch_bounds__(256) void clip_gather_kernel(ClipArgs a) {
    const long long total = a.n3 + a.n2 + a.ncam;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (i < a.n3) {
            clip_quad<3>(a.seq3d, a.out3d, i, a, a.perm3d, a.frames3, a.shift3);
        } else if (i < a.n3 + a.n2) {
            clip_quad<2>(a.seq2d, a.out2d, i - a.n3, a, a.perm2d, a.frames2, a.shift2);
        } else {
            const long long k = i - a.n3 - a.n2;
            const int rec = (int)(k / a.cam_w), c = (int)(k - (long long)rec * a.cam_w);
            const int4 r = a.records[rec];
            const float x = a.cams[(long long)r.x * a.cam_w + c];
            a.out_cam[k] = (r.w != 0 && (c == 2 || c == 7)) ? -x : x;   // flipped principal point / tangential p1
        }
    }
}

// ---------------------------------------------------------------------------------------------------- clip pair batch
// dhaug_pair_batch (dhaug_posetrain.hip) reading its rows straight from the resident sequences: one pose-frame per lane, the 3D
// frames first, then the 2D frames.  An unflipped record's frame is 12 / 8 float4 loads; a flipped record's frame is loaded joint
// by joint through the packed permutation (the run-time index is in the ADDRESS, the register array keeps constant indices), the
// training flip is the compile-time one of dhaug_pose_regs.h.  Small workgroups and the same cap as pair_batch_kernel.
constexpr int kClipPairBlock = 64;
constexpr int kClipPairMaxGrid = 2048;

struct ClipPairArgs {
    const float* seq3d;
    const float* seq2d;
    const long long* seq_offset;
    const int* seq_len;
    const int4* records;
    float* tgt;
    float* tgt_flip;
    float* inp;
    float* inp_flip;
    float* inp_back;
    float* inp_flip_back;
    unsigned long long perm3d, perm2d;
    long long n3, n2;             // pose-frames of the 3D / 2D outputs (0 when none of that kind is asked for)
    int frames3, shift3, frames2, shift2;
};

// one source frame into registers with the record's flip applied
template <int C>
__device__ __forceinline__ void load_clip_pose(const float* __restrict__ s, bool flip, unsigned long long perm, float (&x)[16 * C]) {
    if (!flip) {
        dhaug_pose_regs::load_pose<C>(s, x);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float* sj = s + C * (int)((perm >> (4 * j)) & 15u);
            x[C * j] = -sj[0];
#pragma unroll
            for (int c = 1; c < C; ++c) x[C * j + c] = sj[c];
        }
    }
}

__global__ __launch_bounds__(kClipPairBlock) void clip_pair_batch_kernel(ClipPairArgs a) {
    using namespace dhaug_pose_regs;
    const long long total = a.n3 + a.n2;
    for (long long item = (long long)blockIdx.x * kClipPairBlock + threadIdx.x; item < total;
         item += (long long)gridDim.x * kClipPairBlock) {
        if (item < a.n3) {
            const int it = (int)item, rec = it / a.frames3, f = it - rec * a.frames3;
            const int4 r = a.records[rec];
            float x[48], y[48];
            load_clip_pose<3>(a.seq3d + clip_frame(a.seq_offset, a.seq_len, r, a.shift3, f) * 48, r.w != 0, a.perm3d, x);
            const float r0 = x[0], r1 = x[1], r2 = x[2];
#pragma unroll
            for (int j = 0; j < 16; ++j) { x[3 * j] -= r0; x[3 * j + 1] -= r1; x[3 * j + 2] -= r2; }
            if (a.tgt) store_pose<3>(a.tgt + item * 48, x);
            if (a.tgt_flip) { flip_pose<3>(x, y); store_pose<3>(a.tgt_flip + item * 48, y); }
        } else {
            const long long it2 = item - a.n3;
            const int rec = (int)it2 / a.frames2, f = (int)it2 - rec * a.frames2;
            const int4 r = a.records[rec];
            const long long back = ((long long)rec * a.frames2 + (a.frames2 - 1 - f)) * 32;
            float x[32], y[32];
            load_clip_pose<2>(a.seq2d + clip_frame(a.seq_offset, a.seq_len, r, a.shift2, f) * 32, r.w != 0, a.perm2d, x);
            if (a.inp) store_pose<2>(a.inp + it2 * 32, x);
            if (a.inp_back) store_pose<2>(a.inp_back + back, x);
            if (a.inp_flip || a.inp_flip_back) {
                flip_pose<2>(x, y);
                if (a.inp_flip) store_pose<2>(a.inp_flip + it2 * 32, y);
                if (a.inp_flip_back) store_pose<2>(a.inp_flip_back + back, y);
            }
        }
    }
}

// host perm[16] -> packed nibbles; NULL = identity; anything but a permutation of 0..15 -> false
bool pack_perm(const int8_t* perm, unsigned long long& out) {
    out = 0;
    unsigned seen = 0;
    for (int j = 0; j < 16; ++j) {
        const int p = perm ? perm[j] : j;
        if (p < 0 || p >= 16 || (seen >> p) & 1u) return false;
        seen |= 1u << p;
        out |= (unsigned long long)p << (4 * j);
    }
    return true;
}

// output rows are indexed in 32 bits (a batch of 2^31 clip frames would be 400 GB of output)
bool rows_fit(int64_t nrec, int frames) { return nrec < (1ll << 31) && nrec * (long long)frames < (1ll << 31) / 12; }
bool shift_fits(long long shift) { return shift < (1ll << 30) && shift > -(1ll << 30); }

// both gather entry points behind their own first checks
int clip_gather_launch(const float* seq3d, const float* seq2d, const float* cams, int cam_w, const int64_t* seq_offset,
                       const int32_t* seq_len, const int32_t* records, int64_t nrec, int frames3, long long shift3, int frames2,
                       long long shift2, const int8_t* perm3d, const int8_t* perm2d, float* out3d, float* out2d, float* out_cam,
                       void* stream) {
    DHAUG_CHECK((seq3d == nullptr) == (out3d == nullptr), DHAUG_EINVAL);
    DHAUG_CHECK((cams == nullptr) == (out_cam == nullptr), DHAUG_EINVAL);
    DHAUG_CHECK(cams == nullptr || cam_w >= 1, DHAUG_EINVAL);
    ClipArgs a;
    DHAUG_CHECK(pack_perm(perm3d, a.perm3d) && pack_perm(perm2d, a.perm2d), DHAUG_EINVAL);
    if (nrec == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(seq2d); DHAUG_CHECK_PTR(out2d); DHAUG_CHECK_PTR(seq_offset); DHAUG_CHECK_PTR(seq_len);
    DHAUG_CHECK_PTR(records);
    DHAUG_CHECK(rows_fit(nrec, frames3) && rows_fit(nrec, frames2) && shift_fits(shift3) && shift_fits(shift2), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(dhaug_aligned16(seq2d) && dhaug_aligned16(out2d) && dhaug_aligned16(records), DHAUG_EALIGN);
    DHAUG_CHECK(seq3d == nullptr || (dhaug_aligned16(seq3d) && dhaug_aligned16(out3d)), DHAUG_EALIGN);
    DHAUG_CHECK(cams == nullptr || ((uintptr_t)cams % 4 == 0 && (uintptr_t)out_cam % 4 == 0), DHAUG_EALIGN);
    a.seq3d = seq3d; a.seq2d = seq2d; a.cams = cams;
    a.seq_offset = reinterpret_cast<const long long*>(seq_offset);
    a.seq_len = seq_len;
    a.records = reinterpret_cast<const int4*>(records);
    a.out3d = out3d; a.out2d = out2d; a.out_cam = out_cam;
    a.n3 = seq3d ? nrec * (long long)frames3 * 12 : 0;
    a.n2 = nrec * (long long)frames2 * 8;
    a.ncam = cams ? nrec * (long long)cam_w : 0;
    a.frames3 = frames3; a.shift3 = (int)shift3; a.frames2 = frames2; a.shift2 = (int)shift2; a.cam_w = cams ? cam_w : 1;
    const long long items = a.n3 + a.n2 + a.ncam;
    long long blocks = (items + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(clip_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return dhaug_launch_status();
}

}  // namespace

extern "C" int dhaug_clip_gather(const float* seq3d, const float* seq2d, const float* cams, int cam_w,
                                 const int64_t* seq_offset, const int32_t* seq_len, const int32_t* records, int64_t nrec,
                                 int frames, int pad, int causal_shift, const int8_t* perm3d, const int8_t* perm2d,
                                 float* out3d, float* out2d, float* out_cam, void* stream) {
    DHAUG_CHECK(nrec >= 0 && frames >= 1 && pad >= 0, DHAUG_EINVAL);
    const long long shift = (long long)pad + causal_shift;
    return clip_gather_launch(seq3d, seq2d, cams, cam_w, seq_offset, seq_len, records, nrec, frames, shift, frames, shift, perm3d,
                              perm2d, out3d, out2d, out_cam, stream);
}

extern "C" int dhaug_clip_gather_windows(const float* seq3d, const float* seq2d, const float* cams, int cam_w,
                                         const int64_t* seq_offset, const int32_t* seq_len, const int32_t* records, int64_t nrec,
                                         int frames3, int shift3, int frames2, int shift2, const int8_t* perm3d,
                                         const int8_t* perm2d, float* out3d, float* out2d, float* out_cam, void* stream) {
    DHAUG_CHECK(nrec >= 0 && frames3 >= 1 && frames2 >= 1, DHAUG_EINVAL);
    return clip_gather_launch(seq3d, seq2d, cams, cam_w, seq_offset, seq_len, records, nrec, frames3, shift3, frames2, shift2,
                              perm3d, perm2d, out3d, out2d, out_cam, stream);
}

extern "C" int dhaug_clip_pair_batch(const float* seq3d, const float* seq2d, const int64_t* seq_offset, const int32_t* seq_len,
                                     const int32_t* records, int64_t nrec, int frames3, int shift3, int frames2, int shift2,
                                     const int8_t* perm3d, const int8_t* perm2d, int flip, int playback, float* tgt, float* inp,
                                     float* tgt_flip, float* inp_flip, float* inp_back, float* inp_flip_back, void* stream) {
    DHAUG_CHECK(nrec >= 0 && frames3 >= 1 && frames2 >= 1, DHAUG_EINVAL);
    DHAUG_CHECK(flip || (!tgt_flip && !inp_flip && !inp_flip_back), DHAUG_EINVAL);
    DHAUG_CHECK(playback || (!inp_back && !inp_flip_back), DHAUG_EINVAL);
    const bool want3 = tgt || tgt_flip, want2 = inp || inp_flip || inp_back || inp_flip_back;
    DHAUG_CHECK(want3 || want2, DHAUG_EINVAL);
    DHAUG_CHECK((!want3 || seq3d) && (!want2 || seq2d), DHAUG_EINVAL);
    ClipPairArgs a;
    DHAUG_CHECK(pack_perm(perm3d, a.perm3d) && pack_perm(perm2d, a.perm2d), DHAUG_EINVAL);
    if (nrec == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(seq_offset); DHAUG_CHECK_PTR(seq_len); DHAUG_CHECK_PTR(records);
    DHAUG_CHECK(rows_fit(nrec, frames3) && rows_fit(nrec, frames2) && shift_fits(shift3) && shift_fits(shift2), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(dhaug_aligned16(seq3d) && dhaug_aligned16(seq2d) && dhaug_aligned16(records) && dhaug_aligned16(tgt) &&
                dhaug_aligned16(inp) && dhaug_aligned16(tgt_flip) && dhaug_aligned16(inp_flip) && dhaug_aligned16(inp_back) &&
                dhaug_aligned16(inp_flip_back) && (reinterpret_cast<uintptr_t>(seq_offset) & 7u) == 0 &&
                (reinterpret_cast<uintptr_t>(seq_len) & 3u) == 0, DHAUG_EALIGN);
    a.seq3d = seq3d; a.seq2d = seq2d;
    a.seq_offset = reinterpret_cast<const long long*>(seq_offset);
    a.seq_len = seq_len;
    a.records = reinterpret_cast<const int4*>(records);
    a.tgt = tgt; a.tgt_flip = tgt_flip; a.inp = inp; a.inp_flip = inp_flip; a.inp_back = inp_back; a.inp_flip_back = inp_flip_back;
    a.n3 = want3 ? nrec * (long long)frames3 : 0;
    a.n2 = want2 ? nrec * (long long)frames2 : 0;
    a.frames3 = frames3; a.shift3 = shift3; a.frames2 = frames2; a.shift2 = shift2;
    hipLaunchKernelGGL(clip_pair_batch_kernel, dim3(dhaug_stream_grid(a.n3 + a.n2, kClipPairBlock, kClipPairMaxGrid)),
                       dim3(kClipPairBlock), 0, (hipStream_t)stream, a);
    return dhaug_launch_status();
}
