// Clip gather of the video GAN's real-data loader (GAN_video_ChunkedGenerator.next_epoch,
// R/models_Fk_GAN/video_mode_operate.py:126-183): one launch writes a whole batch of (frames, 16, C) clips from the
// concatenated device-resident sequences.  Pure data movement -- a copy, a sign flip and a joint permutation -- so the
// output equals the reference's float64 batch cast to fp32 bit for bit.
//
// Work items, one flat index space: the 16-byte quads of the 3D frames (12 per frame), then those of the 2D frames (8 per
// frame), then the camera scalars.  Every store is a 16-byte store of consecutive output addresses (the camera's a 4-byte one);
// an unflipped quad is one 16-byte load of the source frame, a flipped one four scalar loads through the joint permutation.
// A batch is a few MB: latency-bound, one short launch.
#include "dhaug_common.h"

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
    int frames, shift, cam_w;     // shift = pad + causal_shift
};

// source frame (absolute row of the concatenated sequences) of output row `row` = (record, frame); flip flag of the record
__device__ __forceinline__ long long clip_source(const ClipArgs& a, int row, bool& flip) {
    const int rec = row / a.frames, f = row - rec * a.frames;
    const int4 r = a.records[rec];
    flip = r.w != 0;
    const long long last = a.seq_len[r.x] - 1;
    long long t = (long long)r.y - a.shift + f;       // (start - pad - causal_shift) + f, then the 'edge' padding
    t = t < 0 ? 0 : (t > last ? last : t);
    return a.seq_offset[r.x] + t;
}

// quad q (4 floats) of an output frame of 16 joints x W coordinates
template <int W>
__device__ __forceinline__ void clip_quad(const float* __restrict__ seq, float* __restrict__ out, long long i,
                                          const ClipArgs& a, unsigned long long perm) {
    constexpr int QPF = 16 * W / 4;                   // quads per frame: 12 (3D), 8 (2D)
    const int row = (int)(i / QPF), q = (int)(i - (long long)row * QPF);
    bool flip;
    const float* s = seq + clip_source(a, row, flip) * (16 * W);
    float4 v;
    if (!flip) {
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
            clip_quad<3>(a.seq3d, a.out3d, i, a, a.perm3d);
        } else if (i < a.n3 + a.n2) {
            clip_quad<2>(a.seq2d, a.out2d, i - a.n3, a, a.perm2d);
        } else {
            const long long k = i - a.n3 - a.n2;
            const int rec = (int)(k / a.cam_w), c = (int)(k - (long long)rec * a.cam_w);
            const int4 r = a.records[rec];
            const float x = a.cams[(long long)r.x * a.cam_w + c];
            a.out_cam[k] = (r.w != 0 && (c == 2 || c == 7)) ? -x : x;   // flipped principal point / tangential p1
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

}  // namespace

extern "C" int dhaug_clip_gather(const float* seq3d, const float* seq2d, const float* cams, int cam_w,
                                 const int64_t* seq_offset, const int32_t* seq_len, const int32_t* records, int64_t nrec,
                                 int frames, int pad, int causal_shift, const int8_t* perm3d, const int8_t* perm2d,
                                 float* out3d, float* out2d, float* out_cam, void* stream) {
    DHAUG_CHECK(nrec >= 0 && frames >= 1 && pad >= 0, DHAUG_EINVAL);
    DHAUG_CHECK((seq3d == nullptr) == (out3d == nullptr), DHAUG_EINVAL);
    DHAUG_CHECK((cams == nullptr) == (out_cam == nullptr), DHAUG_EINVAL);
    DHAUG_CHECK(cams == nullptr || cam_w >= 1, DHAUG_EINVAL);
    ClipArgs a;
    DHAUG_CHECK(pack_perm(perm3d, a.perm3d) && pack_perm(perm2d, a.perm2d), DHAUG_EINVAL);
    if (nrec == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(seq2d); DHAUG_CHECK_PTR(out2d); DHAUG_CHECK_PTR(seq_offset); DHAUG_CHECK_PTR(seq_len);
    DHAUG_CHECK_PTR(records);
    // output rows are indexed in 32 bits (a batch of 2^31 clip frames would be 400 GB of output)
    DHAUG_CHECK(nrec < (1ll << 31) && nrec * (long long)frames < (1ll << 31) / 12 && (long long)pad + causal_shift < (1ll << 30) &&
                (long long)pad + causal_shift > -(1ll << 30), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(dhaug_aligned16(seq2d) && dhaug_aligned16(out2d) && dhaug_aligned16(records), DHAUG_EALIGN);
    DHAUG_CHECK(seq3d == nullptr || (dhaug_aligned16(seq3d) && dhaug_aligned16(out3d)), DHAUG_EALIGN);
    DHAUG_CHECK(cams == nullptr || ((uintptr_t)cams % 4 == 0 && (uintptr_t)out_cam % 4 == 0), DHAUG_EALIGN);
    a.seq3d = seq3d; a.seq2d = seq2d; a.cams = cams;
    a.seq_offset = reinterpret_cast<const long long*>(seq_offset);
    a.seq_len = seq_len;
    a.records = reinterpret_cast<const int4*>(records);
    a.out3d = out3d; a.out2d = out2d; a.out_cam = out_cam;
    const long long rows = nrec * (long long)frames;
    a.n3 = seq3d ? rows * 12 : 0;
    a.n2 = rows * 8;
    a.ncam = cams ? nrec * (long long)cam_w : 0;
    a.frames = frames; a.shift = pad + causal_shift; a.cam_w = cams ? cam_w : 1;
    const long long items = a.n3 + a.n2 + a.ncam;
    long long blocks = (items + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(clip_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return dhaug_launch_status();
}
