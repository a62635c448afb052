// The arithmetic of the SemGCN posenet that no other file has (R/models_baseline/gcn/sem_graph_conv.py SemGraphConv.forward): the mix of
// the 16 joints of every pose through a 16 x 16 adjacency, between the layer's dense product and its BatchNorm.  Activations are rows
// (pose-major, then joint): row 16 b + i is joint i of pose b.
//
//  dhaug_graph_mix       z[b,i,:] = A[i,i] h0[b,i,:] + sum_{j != i} A[i,j] h1[b,j,:] + bias, H = [h0 | h1] one (M, 2C) matrix; with
//                        transpose = 1 the adjoint, dh0[b,i,:] = A[i,i] g[b,i,:], dh1[b,j,:] = sum_{i != j} A[i,j] g[b,i,:].
//  dhaug_graph_adj_grad  dA[i,j] = sum_{b,c} g[b,i,c] (i == j ? h0 : h1)[b,j,c] at the listed pairs, exactly 0 elsewhere: per-workgroup
//                        fp64 partials, then a second launch that adds them in workgroup order.
//  dhaug_graph_wcat      W (2, in, out) <-> Wcat (2 out, in) = [W[0]^T ; W[1]^T], the B operand of H = x Wcat^T, and its adjoint.
//
// Mix: one work item = one pose x one channel vector of N = 4 (fp32 source) or 8 (bf16 source) channels; adjacent lanes own adjacent
// vectors of a pose, so the 64 lanes of a wave read and write whole row segments.  The item keeps the 16 rows it mixes in registers
// (h1, or g for the adjoint), streams the diagonal operand, and writes one output row per joint; A lies in LDS (every lane reads the
// same word: a broadcast).  Sums run j (i) ascending behind the diagonal term, explicit fmaf, fp32; one rounding on a bf16 output.
// Alignment: the 16-byte accesses are taken only where the kernel itself finds both base addresses, both row pitches and C * element
// size on the 16-byte grid (one uniform test per launch, the rule of dhaug_split_bf16); everything else goes element by element.  A
// and bias are ALWAYS read element by element: the optimizer's flat buffer places tensors of odd size (the 46-element e, the
// 3-element output bias) on 4-byte boundaries.  No atomics, IEEE semantics: the same call gives the same bits.
#include "dhaug_common.h"

namespace {

constexpr int kJoints = 16;
constexpr int kMixBlock = 256;
constexpr int kMixMaxBlocks = DHAUG_GRAPH_MIX_MAX_BLOCKS;
constexpr int kAdjBlock = 256;
constexpr int kAdjMaxBlocks = DHAUG_GRAPH_ADJ_MAX_BLOCKS;
constexpr int kMaxPairs = DHAUG_GRAPH_MAX_PAIRS;

template <typename T> struct VecOf;
template <> struct VecOf<float> { static constexpr int N = 4; };
template <> struct VecOf<uint16_t> { static constexpr int N = 8; };

// the first `valid` (<= N) of N consecutive elements at p, the rest 0; `whole`: one 16-byte load (the caller has tested alignment)
__device__ __forceinline__ void load_vec(const float* __restrict__ p, bool whole, int valid, float (&v)[4]) {
    if (whole) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < valid ? p[k] : 0.0f;
    }
}
__device__ __forceinline__ void load_vec(const uint16_t* __restrict__ p, bool whole, int valid, float (&v)[8]) {
    if (whole) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = __builtin_bit_cast(float, w[k] << 16);
            v[2 * k + 1] = __builtin_bit_cast(float, w[k] & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = k < valid ? dhaug_bf16_to_f32(p[k]) : 0.0f;
    }
}

__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    return (unsigned)dhaug_f32_to_bf16(lo) | ((unsigned)dhaug_f32_to_bf16(hi) << 16);
}
// the first `count` (<= N) of N values to p; `whole`: vector stores (count == N, alignment tested by the caller)
template <int N>
__device__ __forceinline__ void store_vec(float* __restrict__ p, bool whole, int count, const float (&v)[N]) {
    if (whole) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < count) p[k] = v[k];
    }
}
template <int N>
__device__ __forceinline__ void store_vec(uint16_t* __restrict__ p, bool whole, int count, const float (&v)[N]) {
    if (whole) {
        if constexpr (N == 8)
            *reinterpret_cast<uint4*>(p) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        else
            *reinterpret_cast<uint2*>(p) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < count) p[k] = dhaug_f32_to_bf16(v[k]);
    }
}

struct MixArgs {
    const void* src;            // forward: H (M, ld_src >= 2C); adjoint: g (M, ld_src >= C)
    void* dst;                  // forward: z (M, ld_dst >= cw); adjoint: dH (M, ld_dst >= C + cw)
    const float* A;             // 16 x 16, row-major
    const float* bias;          // C, or null (forward only)
    long long ld_src, ld_dst, poses, C;
    long long cw;               // columns an item may own: C, on a bf16 output up to the end of the zero pad
    long long nv;               // channel vectors per pose: ceil(cw / N)
    int vec;                    // the host found every pitch and C on the 16-byte grid (the kernel tests the addresses)
};

template <typename TI, typename TO, bool TR>
__global__ __launch_bounds__(kMixBlock) void graph_mix_kernel(MixArgs a) {
    constexpr int N = VecOf<TI>::N;
    __shared__ float As[kJoints][kJoints];
    As[threadIdx.x >> 4][threadIdx.x & 15] = a.A[threadIdx.x];          // (kMixBlock == 256 == 16 x 16: one element per thread)
    __syncthreads();
    const TI* src = reinterpret_cast<const TI*>(a.src);
    TO* dst = reinterpret_cast<TO*>(a.dst);
    const long long C = a.C;
    const bool vec = a.vec && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const long long items = a.poses * a.nv, stride = (long long)gridDim.x * kMixBlock;
    for (long long it = (long long)blockIdx.x * kMixBlock + threadIdx.x; it < items; it += stride) {
        const long long b = it / a.nv, col = (it - b * a.nv) * N;
        const long long left = C - col;                                  // channels of this vector that exist (<= 0: all pad)
        const int valid = left >= N ? N : (left > 0 ? (int)left : 0);
        const long long room = a.cw - col;
        const int count = room >= N ? N : (int)room;                     // columns of this vector that are written (pad included)
        const bool whole_in = vec && valid == N, whole_out = vec && count == N;
        const TI* s = src + b * kJoints * a.ld_src + col;
        TO* d = dst + b * kJoints * a.ld_dst + col;
        float keep[kJoints][N];                                          // forward: h1 rows; adjoint: g rows
#pragma unroll
        for (int j = 0; j < kJoints; ++j) {
            if (valid) load_vec(s + j * a.ld_src + (TR ? 0 : C), whole_in, valid, keep[j]);
            else {
#pragma unroll
                for (int k = 0; k < N; ++k) keep[j][k] = 0.0f;
            }
        }
        // the joint loops below stay rolled: the kept rows are indexed by the inner (unrolled) loop only, and a weight of the rolled
        // index is read from LDS when it is used (unrolled, the compiler hoists all 256 of them into registers and spills the rows).
        // The term of the diagonal's own row enters the off-diagonal sum with weight 0, as in the reference's dense products.
        if (!TR) {
            float bv[N];
#pragma unroll
            for (int k = 0; k < N; ++k) bv[k] = (a.bias != nullptr && k < valid) ? a.bias[col + k] : 0.0f;
#pragma unroll 1
            for (int i = 0; i < kJoints; ++i) {
                float h0[N] = {}, z[N];
                if (valid) load_vec(s + i * a.ld_src, whole_in, valid, h0);
#pragma unroll
                for (int k = 0; k < N; ++k) z[k] = As[i][i] * h0[k];
#pragma unroll
                for (int j = 0; j < kJoints; ++j) {
                    const float w = j == i ? 0.0f : As[i][j];
#pragma unroll
                    for (int k = 0; k < N; ++k) z[k] = fmaf(w, keep[j][k], z[k]);
                }
#pragma unroll
                for (int k = 0; k < N; ++k) z[k] = k < valid ? z[k] + bv[k] : 0.0f;
                store_vec<N>(d + i * a.ld_dst, whole_out, count, z);
            }
        } else {
#pragma unroll 1
            for (int j = 0; j < kJoints; ++j) {
                float gj[N] = {}, d0[N], d1[N];
                if (valid) load_vec(s + j * a.ld_src, whole_in, valid, gj);
#pragma unroll
                for (int k = 0; k < N; ++k) { d0[k] = As[j][j] * gj[k]; d1[k] = 0.0f; }
#pragma unroll
                for (int i = 0; i < kJoints; ++i) {
                    const float w = i == j ? 0.0f : As[i][j];
#pragma unroll
                    for (int k = 0; k < N; ++k) d1[k] = fmaf(w, keep[i][k], d1[k]);
                }
#pragma unroll
                for (int k = 0; k < N; ++k)
                    if (k >= valid) d1[k] = 0.0f;                        // (the pad behind dh1: zeros, whatever A holds)
                if (valid) store_vec<N>(d + j * a.ld_dst, whole_in, valid, d0);
                store_vec<N>(d + j * a.ld_dst + C, whole_out, count, d1);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ adjacency gradient
struct AdjArgs {
    const void* g;
    const void* h;
    const int* pairs;           // nnz x (i, j)
    double* ws;                 // (blocks, kMaxPairs)
    long long ld_g, ld_h, poses, C, poses_per_block;
    int nnz, g_bf16, h_bf16;
};

__device__ __forceinline__ float elem(const void* p, int bf16, long long idx) {
    return bf16 ? dhaug_bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[idx]) : reinterpret_cast<const float*>(p)[idx];
}

// a wave owns every fourth pair; for one pair its lanes stride over the channels and walk the workgroup's poses, each lane summing its
// products in fp64 in that order; the 64 lane sums are added by a butterfly (the same tree in every call), lane 0 writes the partial
__global__ __launch_bounds__(kAdjBlock) void graph_adj_partials_kernel(AdjArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long b0 = (long long)blockIdx.x * a.poses_per_block;
    const long long b1 = b0 + a.poses_per_block < a.poses ? b0 + a.poses_per_block : a.poses;
    for (int p = wave; p < a.nnz; p += kAdjBlock / 64) {
        const int i = a.pairs[2 * p], j = a.pairs[2 * p + 1];
        double s = 0.0;
        if (i >= 0 && i < kJoints && j >= 0 && j < kJoints) {           // (a pair outside the 16 joints names no row: its entry stays 0)
            const long long off = i == j ? 0 : a.C;
            for (long long b = b0; b < b1; ++b) {
                const long long rg = (b * kJoints + i) * a.ld_g, rh = (b * kJoints + j) * a.ld_h + off;
                for (long long c = lane; c < a.C; c += 64) s += (double)elem(a.g, a.g_bf16, rg + c) * (double)elem(a.h, a.h_bf16, rh + c);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) a.ws[(long long)blockIdx.x * kMaxPairs + p] = s;
    }
}

// one workgroup: every entry 0, then the listed entries = their partials added in workgroup order
__global__ __launch_bounds__(kMaxPairs) void graph_adj_finish_kernel(const double* __restrict__ ws, const int* __restrict__ pairs, int nnz,
                                                                     int blocks, float* __restrict__ dA) {
    const int t = threadIdx.x;
    dA[t] = 0.0f;                                                        // (kMaxPairs == 256 == 16 x 16 threads)
    __syncthreads();
    if (t < nnz) {
        const int i = pairs[2 * t], j = pairs[2 * t + 1];
        if (i >= 0 && i < kJoints && j >= 0 && j < kJoints) {
            double s = 0.0;
            for (int k = 0; k < blocks; ++k) s += ws[(long long)k * kMaxPairs + t];
            dA[i * kJoints + j] = (float)s;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ W <-> Wcat
// to_cat: dst[(k out + n) in + c] = src[(k in + c) out + n]; otherwise dst[(k in + c) out + n] = src[(k out + n) in + c]
__global__ __launch_bounds__(256) void graph_wcat_kernel(const float* __restrict__ src, float* __restrict__ dst, long long in, long long out,
                                                         int to_cat) {
    const long long total = 2 * in * out, stride = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const long long k = e / (in * out), r = e - k * in * out;
        long long c, n;
        if (to_cat) { n = r / in; c = r - n * in; }
        else { c = r / out; n = r - c * out; }
        const long long cat = (k * out + n) * in + c, w = (k * in + c) * out + n;
        dst[e] = src[to_cat ? w : cat];
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

constexpr int64_t kMaxCols = 1ll << 28;
constexpr int64_t kMaxRows = 1ll << 40;

template <typename TI, typename TO>
void launch_mix(const MixArgs& a, int transpose, unsigned grid, hipStream_t stream) {
    if (transpose)
        hipLaunchKernelGGL((graph_mix_kernel<TI, TO, true>), dim3(grid), dim3(kMixBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((graph_mix_kernel<TI, TO, false>), dim3(grid), dim3(kMixBlock), 0, stream, a);
}

}  // namespace

extern "C" int dhaug_graph_mix(const void* src, int src_bf16, int64_t ld_src, const float* A, const float* bias, void* dst,
                               int dst_bf16, int64_t ld_dst, int64_t M, int64_t C, int transpose, void* stream) {
    DHAUG_CHECK(M >= 0 && C >= 0 && (src_bf16 == 0 || src_bf16 == 1) && (dst_bf16 == 0 || dst_bf16 == 1) &&
                (transpose == 0 || transpose == 1), DHAUG_EINVAL);
    DHAUG_CHECK(M % kJoints == 0, DHAUG_EINVAL);
    if (M == 0 || C == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(src); DHAUG_CHECK_PTR(A); DHAUG_CHECK_PTR(dst);
    DHAUG_CHECK(!(transpose && bias != nullptr), DHAUG_EINVAL);           // the adjoint has no bias term
    DHAUG_CHECK(C < kMaxCols && M < kMaxRows, DHAUG_EUNSUPPORTED);
    const int es = src_bf16 ? 2 : 4, ed = dst_bf16 ? 2 : 4;
    // the columns behind the last result column that a bf16 output pads with zeros: up to the next multiple of 16
    const int64_t width = transpose ? 2 * C : C, wpad = dst_bf16 ? (width + 15) / 16 * 16 : width;
    DHAUG_CHECK(ld_src >= (transpose ? C : 2 * C) && ld_dst >= wpad, DHAUG_EALIGN);
    DHAUG_CHECK(aligned(src, es) && aligned(dst, ed) && aligned(A, 4) && aligned(bias, 4), DHAUG_EALIGN);
    MixArgs a;
    a.src = src; a.dst = dst; a.A = A; a.bias = bias; a.ld_src = ld_src; a.ld_dst = ld_dst; a.poses = M / kJoints; a.C = C;
    a.cw = transpose ? wpad - C : wpad;
    const int n = src_bf16 ? 8 : 4;
    a.nv = (a.cw + n - 1) / n;
    a.vec = (ld_src * es) % 16 == 0 && (ld_dst * ed) % 16 == 0 && (C * es) % 16 == 0 && (C * ed) % 16 == 0;
    const unsigned grid = (unsigned)dhaug_stream_grid(a.poses * a.nv, kMixBlock, kMixMaxBlocks);
    if (src_bf16) {
        if (dst_bf16) launch_mix<uint16_t, uint16_t>(a, transpose, grid, (hipStream_t)stream);
        else launch_mix<uint16_t, float>(a, transpose, grid, (hipStream_t)stream);
    } else {
        if (dst_bf16) launch_mix<float, uint16_t>(a, transpose, grid, (hipStream_t)stream);
        else launch_mix<float, float>(a, transpose, grid, (hipStream_t)stream);
    }
    return dhaug_launch_status();
}

extern "C" int dhaug_graph_adj_grad(const void* g, int g_bf16, int64_t ld_g, const void* h, int h_bf16, int64_t ld_h,
                                    const int32_t* pairs, int nnz, float* dA, void* workspace, int64_t M, int64_t C, void* stream) {
    DHAUG_CHECK(M >= 0 && C >= 0 && (g_bf16 == 0 || g_bf16 == 1) && (h_bf16 == 0 || h_bf16 == 1), DHAUG_EINVAL);
    DHAUG_CHECK(nnz >= 0 && nnz <= kMaxPairs && M % kJoints == 0, DHAUG_EINVAL);
    if (M == 0 || C == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(g); DHAUG_CHECK_PTR(h); DHAUG_CHECK_PTR(dA); DHAUG_CHECK_PTR(workspace);
    DHAUG_CHECK(nnz == 0 || pairs != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(C < kMaxCols && M < kMaxRows, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(ld_g >= C && ld_h >= 2 * C, DHAUG_EALIGN);
    DHAUG_CHECK(aligned(g, g_bf16 ? 2 : 4) && aligned(h, h_bf16 ? 2 : 4) && aligned(pairs, 4) && aligned(dA, 4) && aligned(workspace, 8),
                DHAUG_EALIGN);
    AdjArgs a;
    a.g = g; a.h = h; a.pairs = pairs; a.ws = (double*)workspace; a.ld_g = ld_g; a.ld_h = ld_h; a.poses = M / kJoints; a.C = C;
    a.nnz = nnz; a.g_bf16 = g_bf16; a.h_bf16 = h_bf16;
    const int64_t want = a.poses < kAdjMaxBlocks ? a.poses : kAdjMaxBlocks;
    a.poses_per_block = (a.poses + want - 1) / want;
    const int blocks = (int)((a.poses + a.poses_per_block - 1) / a.poses_per_block);
    if (nnz > 0) {
        hipLaunchKernelGGL(graph_adj_partials_kernel, dim3(blocks), dim3(kAdjBlock), 0, (hipStream_t)stream, a);
        const int rc = dhaug_launch_status();
        if (rc != DHAUG_OK) return rc;
    }
    hipLaunchKernelGGL(graph_adj_finish_kernel, dim3(1), dim3(kMaxPairs), 0, (hipStream_t)stream, (const double*)workspace, pairs, nnz,
                       blocks, dA);
    return dhaug_launch_status();
}

extern "C" int dhaug_graph_wcat(const float* src, float* dst, int64_t in, int64_t out, int to_cat, void* stream) {
    DHAUG_CHECK(in >= 0 && out >= 0 && (to_cat == 0 || to_cat == 1), DHAUG_EINVAL);
    if (in == 0 || out == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(src); DHAUG_CHECK_PTR(dst);
    DHAUG_CHECK(src != dst, DHAUG_EINVAL);
    DHAUG_CHECK(in < kMaxCols && out < kMaxCols && in * out < (1ll << 30), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(aligned(src, 4) && aligned(dst, 4), DHAUG_EALIGN);
    hipLaunchKernelGGL(graph_wcat_kernel, dim3(dhaug_stream_grid(2 * in * out, 256)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       (long long)in, (long long)out, to_cat);
    return dhaug_launch_status();
}
