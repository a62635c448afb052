// Tap layout around the GEMMs of the multi-frame VideoPose posenets (R/models_Fk_GAN/mulit_farme_videopose.py): a k-tap Conv1d over
// rows (batch-major, then time) is the plain product  A W2d^T  with  W2d[n, j Cin + c] = W[n, c, j]  and an A operand whose row is the
// concatenation of the k input rows of the window.  The products run on dhaug_gemm_bf16 / dhaug_gemm_tn_bf16_rows; this file moves data:
//
//  dhaug_conv_taps_pack_bf16     fp32 Conv1d weight (N, Cin, k) -> the bf16 forward operand (N, k Cin) and, optionally, the transposed
//                                operand of the input gradient (k Cin, ceil16 N): W is read once, through an LDS tile of kTileN filters x
//                                kTileC channels x k taps (16-byte loads along W's contiguous axis, 16-byte stores along both outputs').
//  dhaug_conv_taps_permute_f32   fp32 (N, Cin, k) <-> (N, k Cin), the second direction with an optional read-add-write: the layout change
//                                of the split precisions' weights and of every precision's weight gradient.  Any sizes: kPermuteVec
//                                consecutive destination elements per thread, one 16-byte store where the destination allows it.
//  dhaug_tap_gather              the A operand of a k-tap layer with dilation and stride over nseq sequences: kGatherRows output rows per
//                                workgroup pass, 8 elements (one or two 16-byte loads, one to three 16-byte stores) per thread and item.
//
// Vector stores only, no atomics: every thread owns the elements it writes (the accumulate path included).
#include "dhaug_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxTaps = 16;
constexpr int kTileN = 32;                                // filters (rows of W) per pack tile
constexpr int kTileC = 16;                                // input channels per pack tile
constexpr int kTilePitch = kTileC * kMaxTaps + 2;         // uint16 elements per LDS row (odd number of 4-byte banks)
constexpr int kPermuteVec = 4;                            // destination elements per thread of the permute kernel
constexpr int kGatherRows = 8;                            // output rows per workgroup pass of the gather kernel

__device__ __forceinline__ uint4 pack8(const uint16_t (&v)[8]) {
    return make_uint4((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
                      (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16));
}

// One tile: filters [n0, n0 + kTileN) x channels [c0, c0 + kTileC) x all k taps.  In W that is kTileN runs of kTileC * k contiguous
// floats (64 k bytes each, 16-byte aligned: Cin and c0 are multiples of 16).  Filters at and beyond N read as zero, so the nn operand's
// pad columns [N, ceil16 N) come out as zeros.
__global__ __launch_bounds__(kBlock) void taps_pack_kernel(const float* __restrict__ W, uint16_t* __restrict__ nt, long long ld_nt,
                                                           uint16_t* __restrict__ nn, long long ld_nn, int N, int Cin, int k) {
    __shared__ uint16_t t[kTileN][kTilePitch];
    const int tiles_c = Cin / kTileC, tiles_n = (N + kTileN - 1) / kTileN;
    const int n_pad = (N + 15) / 16 * 16;
    const int f4_per_row = kTileC * k / 4;                                         // 4 k
    for (int tile = blockIdx.x; tile < tiles_n * tiles_c; tile += gridDim.x) {
        const int n0 = (tile / tiles_c) * kTileN, c0 = (tile % tiles_c) * kTileC;
        for (int q = threadIdx.x; q < kTileN * f4_per_row; q += kBlock) {
            const int r = q / f4_per_row, f = q - r * f4_per_row;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (n0 + r < N) v = *reinterpret_cast<const float4*>(W + ((long long)(n0 + r) * Cin + c0) * k + 4 * f);
            uint16_t* d = &t[r][4 * f];
            d[0] = dhaug_f32_to_bf16(v.x); d[1] = dhaug_f32_to_bf16(v.y); d[2] = dhaug_f32_to_bf16(v.z); d[3] = dhaug_f32_to_bf16(v.w);
        }
        __syncthreads();
        // nt[n, j Cin + c0 + 8 h .. + 8): two 16-byte stores per (filter, tap)
        for (int i = threadIdx.x; i < kTileN * k * 2; i += kBlock) {
            const int r = i / (2 * k), rem = i - r * 2 * k, j = rem >> 1, h = rem & 1;
            if (n0 + r < N) {
                uint16_t v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = t[r][(8 * h + e) * k + j];
                *reinterpret_cast<uint4*>(nt + (long long)(n0 + r) * ld_nt + (long long)j * Cin + c0 + 8 * h) = pack8(v);
            }
        }
        // nn[j Cin + c0 + c, n0 + 8 g .. + 8): kTileN / 8 16-byte stores per (tap, channel)
        if (nn != nullptr) {
            constexpr int groups = kTileN / 8;
            for (int i = threadIdx.x; i < k * kTileC * groups; i += kBlock) {
                const int g = i % groups, cj = i / groups, c = cj % kTileC, j = cj / kTileC;
                if (n0 + 8 * g < n_pad) {
                    uint16_t v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = t[8 * g + e][c * k + j];
                    *reinterpret_cast<uint4*>(nn + ((long long)j * Cin + c0 + c) * ld_nn + n0 + 8 * g) = pack8(v);
                }
            }
        }
        __syncthreads();
    }
}

// flat destination index e -> flat source index.  Both matrices are contiguous: (N, Cin, k) and (N, k Cin) have N rows of Cin k floats.
template <bool ToTaps>
__device__ __forceinline__ unsigned permute_src(unsigned e, unsigned Cin, unsigned k) {
    const unsigned row = Cin * k, n = e / row, r = e - n * row;
    if (ToTaps) { const unsigned j = r / Cin, c = r - j * Cin; return n * row + c * k + j; }       // dst (n, j, c) <- src (n, c, j)
    const unsigned c = r / k, j = r - c * k;                                                         // dst (n, c, j) <- src (n, j, c)
    return n * row + j * Cin + c;
}

template <bool ToTaps>
__global__ __launch_bounds__(kBlock) void taps_permute_kernel(const float* __restrict__ src, float* __restrict__ dst, unsigned total,
                                                              unsigned Cin, unsigned k, int accumulate) {
    const unsigned groups = (total + kPermuteVec - 1) / kPermuteVec;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < groups; i += gridDim.x * kBlock) {
        const unsigned e0 = i * kPermuteVec;
        if (e0 + kPermuteVec <= total) {
            float4 v = make_float4(src[permute_src<ToTaps>(e0, Cin, k)], src[permute_src<ToTaps>(e0 + 1, Cin, k)],
                                   src[permute_src<ToTaps>(e0 + 2, Cin, k)], src[permute_src<ToTaps>(e0 + 3, Cin, k)]);
            float4* d = reinterpret_cast<float4*>(dst + e0);
            if (accumulate) { const float4 o = *d; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
            *d = v;
        } else {
            for (unsigned e = e0; e < total; ++e) {
                const float v = src[permute_src<ToTaps>(e, Cin, k)];
                dst[e] = accumulate ? dst[e] + v : v;
            }
        }
    }
}

// 8 consecutive elements of an input row as they are (bf16) or as fp32 values
__device__ __forceinline__ void load8(const uint16_t* __restrict__ p, uint4& raw) { raw = *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void load8(const float* __restrict__ p, float4& a, float4& b) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
}

// out[(s t_out + t), j C + c] = x[(s t_in + t stride + j dilation), c]: items of 8 columns, kGatherRows output rows per pass
template <bool XBf16>
__global__ __launch_bounds__(kBlock) void tap_gather_kernel(const void* __restrict__ x_, long long ld_x, long long rows_out, int t_in,
                                                            int t_out, int C, int k, int dilation, int stride,
                                                            uint16_t* __restrict__ ob, long long ld_ob, float* __restrict__ of,
                                                            long long ld_of) {
    const int c8 = C >> 3, per_row = k * c8;
    const long long passes = (rows_out + kGatherRows - 1) / kGatherRows;
    for (long long pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        for (int i = threadIdx.x; i < kGatherRows * per_row; i += kBlock) {
            const int rr = i / per_row, u = i - rr * per_row, j = u / c8, c = (u - j * c8) * 8;
            const long long ro = pass * kGatherRows + rr;
            if (ro >= rows_out) break;                                             // (rr grows with i)
            const long long s = ro / t_out, t = ro - s * t_out;
            const long long ri = s * t_in + t * stride + (long long)j * dilation;  // < (s + 1) t_in: t stride + (k - 1) dilation <= t_in - 1
            const long long oc = (long long)j * C + c;
            if constexpr (XBf16) {
                uint4 raw;
                load8(reinterpret_cast<const uint16_t*>(x_) + ri * ld_x + c, raw);
                *reinterpret_cast<uint4*>(ob + ro * ld_ob + oc) = raw;
            } else {
                float4 a, b;
                load8(reinterpret_cast<const float*>(x_) + ri * ld_x + c, a, b);
                if (of != nullptr) {
                    *reinterpret_cast<float4*>(of + ro * ld_of + oc) = a;
                    *reinterpret_cast<float4*>(of + ro * ld_of + oc + 4) = b;
                }
                if (ob != nullptr) {
                    const uint16_t v[8] = {dhaug_f32_to_bf16(a.x), dhaug_f32_to_bf16(a.y), dhaug_f32_to_bf16(a.z), dhaug_f32_to_bf16(a.w),
                                           dhaug_f32_to_bf16(b.x), dhaug_f32_to_bf16(b.y), dhaug_f32_to_bf16(b.z), dhaug_f32_to_bf16(b.w)};
                    *reinterpret_cast<uint4*>(ob + ro * ld_ob + oc) = pack8(v);
                }
            }
        }
    }
}

constexpr int64_t kMaxIndex = (int64_t)1 << 31;

}  // namespace

extern "C" int dhaug_conv_taps_pack_bf16(const float* W, int64_t N, int64_t Cin, int k, uint16_t* nt, int64_t ld_nt, uint16_t* nn,
                                         int64_t ld_nn, void* stream) {
    DHAUG_CHECK(N >= 0 && Cin >= 0, DHAUG_EINVAL);
    if (N == 0 || Cin == 0) return DHAUG_OK;
    DHAUG_CHECK(k >= 1 && k <= kMaxTaps && Cin % 16 == 0, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(N * Cin * k < kMaxIndex && (Cin * k) * ld_nn < kMaxIndex * 16 && N * ld_nt < kMaxIndex * 16, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK_PTR(W); DHAUG_CHECK_PTR(nt);
    const int64_t n_pad = (N + 15) / 16 * 16;
    DHAUG_CHECK(ld_nt >= Cin * k && (nn == nullptr || ld_nn >= n_pad), DHAUG_EINVAL);
    DHAUG_CHECK(dhaug_aligned16(W) && dhaug_aligned16(nt) && ld_nt % 8 == 0 && (nn == nullptr || (dhaug_aligned16(nn) && ld_nn % 8 == 0)),
                DHAUG_EALIGN);
    const int64_t tiles = ((N + kTileN - 1) / kTileN) * (Cin / kTileC);
    hipLaunchKernelGGL(taps_pack_kernel, dim3(dhaug_stream_grid(tiles, 1)), dim3(kBlock), 0, (hipStream_t)stream, W, nt, (long long)ld_nt,
                       nn, (long long)ld_nn, (int)N, (int)Cin, k);
    return dhaug_launch_status();
}

extern "C" int dhaug_conv_taps_permute_f32(const float* src, float* dst, int64_t N, int64_t Cin, int k, int to_taps, int accumulate,
                                           void* stream) {
    DHAUG_CHECK(N >= 0 && Cin >= 0 && k >= 0 && (to_taps == 0 || to_taps == 1) && (accumulate == 0 || accumulate == 1), DHAUG_EINVAL);
    DHAUG_CHECK(!(to_taps == 1 && accumulate == 1), DHAUG_EINVAL);
    if (N == 0 || Cin == 0 || k == 0) return DHAUG_OK;
    DHAUG_CHECK(N < kMaxIndex && Cin < kMaxIndex && N * Cin < kMaxIndex && N * Cin * k < kMaxIndex, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK_PTR(src); DHAUG_CHECK_PTR(dst);
    DHAUG_CHECK(src != dst, DHAUG_EINVAL);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && dhaug_aligned16(dst), DHAUG_EALIGN);
    const int64_t total = N * Cin * k;
    const dim3 grid(dhaug_stream_grid((total + kPermuteVec - 1) / kPermuteVec, kBlock));
    if (to_taps)
        hipLaunchKernelGGL(taps_permute_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, src, dst, (unsigned)total, (unsigned)Cin,
                           (unsigned)k, accumulate);
    else
        hipLaunchKernelGGL(taps_permute_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, src, dst, (unsigned)total, (unsigned)Cin,
                           (unsigned)k, accumulate);
    return dhaug_launch_status();
}

extern "C" int dhaug_tap_gather(const void* x, int x_bf16, int64_t ld_x, int64_t nseq, int64_t t_in, int64_t C, int k, int dilation,
                                int stride, uint16_t* out_bf16, int64_t ld_ob, float* out_f32, int64_t ld_of, void* stream) {
    DHAUG_CHECK(nseq >= 0 && t_in >= 0 && C >= 0 && (x_bf16 == 0 || x_bf16 == 1) && dilation >= 1 && stride >= 1, DHAUG_EINVAL);
    if (nseq == 0 || C == 0) return DHAUG_OK;
    DHAUG_CHECK(k >= 1 && k <= kMaxTaps && C % 16 == 0, DHAUG_EUNSUPPORTED);
    const int64_t span = (int64_t)(k - 1) * dilation + 1;
    DHAUG_CHECK(t_in >= span, DHAUG_EUNSUPPORTED);                                 // t_out >= 1
    const int64_t t_out = (t_in - span) / stride + 1;
    // index ranges: rows and row items in 32 bits, element offsets in 64
    DHAUG_CHECK(t_in < kMaxIndex && C * k < kMaxIndex / 8 && nseq < kMaxIndex && nseq * t_in < kMaxIndex && dilation < (1 << 30) &&
                stride < (1 << 30), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK_PTR(x);
    DHAUG_CHECK(out_bf16 != nullptr || out_f32 != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(!(x_bf16 == 1 && out_f32 != nullptr), DHAUG_EINVAL);               // fp32 output needs fp32 input
    DHAUG_CHECK(ld_x >= C && (out_bf16 == nullptr || ld_ob >= C * k) && (out_f32 == nullptr || ld_of >= C * k), DHAUG_EINVAL);
    DHAUG_CHECK(dhaug_aligned16(x) && ld_x % (x_bf16 ? 8 : 4) == 0 && (out_bf16 == nullptr || (dhaug_aligned16(out_bf16) && ld_ob % 8 == 0)) &&
                (out_f32 == nullptr || (dhaug_aligned16(out_f32) && ld_of % 4 == 0)), DHAUG_EALIGN);
    const int64_t rows_out = nseq * t_out;
    const dim3 grid(dhaug_stream_grid((rows_out + kGatherRows - 1) / kGatherRows, 1));
    if (x_bf16)
        hipLaunchKernelGGL(tap_gather_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, x, (long long)ld_x, (long long)rows_out,
                           (int)t_in, (int)t_out, (int)C, k, dilation, stride, out_bf16, (long long)ld_ob, out_f32, (long long)ld_of);
    else
        hipLaunchKernelGGL(tap_gather_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, x, (long long)ld_x, (long long)rows_out,
                           (int)t_in, (int)t_out, (int)C, k, dilation, stride, out_bf16, (long long)ld_ob, out_f32, (long long)ld_of);
    return dhaug_launch_status();
}
