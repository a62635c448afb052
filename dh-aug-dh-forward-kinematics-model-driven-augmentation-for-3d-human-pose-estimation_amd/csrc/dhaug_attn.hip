// What the PoseFormer posenet needs between its dense layers (R/models_baseline/poseformer/model_poseformer.py) and no other file has:
// LayerNorm, short-sequence multi-head attention and the exact GELU, each with its backward pass.  Activations are rows; every tensor
// comes with a row pitch; fp32 or bf16 in and out (one rounding from the fp32 result), fp32 arithmetic inside (fp64 for the column sums
// of the LayerNorm parameter gradients).  All row accesses are 4-element vectors (16 bytes of fp32, 8 bytes of bf16): the host checks
// that bases and pitches allow them.  gamma and beta are read element by element: they may lie on any 4-byte boundary (PosenetAdam's
// flat buffer).  No atomics anywhere, every sum runs in a fixed order: the same call gives the same bits.
//
//  LayerNorm   a row is owned by 4, 16 or 64 adjacent lanes of a wave (C <= 128, <= 512, <= 2 048), each lane keeping up to 8 four-element
//              chunks in registers (chunk = lane + k * lanes: the lanes of a row read adjacent 16-byte pieces).  mean = m0 + sum(x - m0) / C
//              with m0 = sum(x) / C (a constant row gives its constant exactly); the centred values then lose their own mean (what fp32
//              cannot hold of the row's), the variance is theirs; butterfly sums.
//              Parameter gradients: workgroups of (32 or 64 columns) x (8 or 4 row lanes) walk a slice of the rows each and write fp64
//              partials, a second launch adds them in workgroup order.
//  Attention   one lane per query row; a workgroup takes as many (sequence, head) pairs as fit 256 lanes and 64 KB of LDS (16 pairs
//              at 16 tokens x 4-wide heads, one at 81 x 64).  K and V of its pairs lie in LDS as fp32; a lane streams the keys in
//              ascending order, all lanes of a pair reading the same LDS row (a broadcast): one pass for the row maximum, one for
//              exp, the denominator and P V.  Backward: phase 1 as the forward (lane = query; P formed again exactly as the forward did, dP =
//              dout . v, D = sum_j P dP, then dS = P (dP - D) and dq) leaves P and dS of the pair in LDS; phase 2 (lane = key) stages Q and dO over K and V and sums dk and dv over the
//              queries in ascending order.
//  GELU        z Phi(z), Phi(z) = erfc(-z / sqrt 2) / 2 (the erf form, not tanh; erfc keeps the far negative tail's relative accuracy,
//              1 + erf(.) cancels there); derivative Phi(z) + z phi(z).  Grid-stride over four-column items.
#include "dhaug_common.h"

namespace {

constexpr int64_t kMaxRows = 1ll << 40;

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// four consecutive elements at element index idx (a multiple of 4 behind a base the host found aligned)
__device__ __forceinline__ void load4(const void* __restrict__ p, int bf16, long long idx, float (&v)[4]) {
    if (bf16) {
        const uint2 t = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(p) + idx);
        v[0] = __builtin_bit_cast(float, t.x << 16); v[1] = __builtin_bit_cast(float, t.x & 0xffff0000u);
        v[2] = __builtin_bit_cast(float, t.y << 16); v[3] = __builtin_bit_cast(float, t.y & 0xffff0000u);
    } else {
        const float4 t = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + idx);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
}
__device__ __forceinline__ void store4(void* __restrict__ p, int bf16, long long idx, const float (&v)[4]) {
    if (bf16) {
        uint2 t;
        t.x = (unsigned)dhaug_f32_to_bf16(v[0]) | ((unsigned)dhaug_f32_to_bf16(v[1]) << 16);
        t.y = (unsigned)dhaug_f32_to_bf16(v[2]) | ((unsigned)dhaug_f32_to_bf16(v[3]) << 16);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p) + idx) = t;
    } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + idx) = make_float4(v[0], v[1], v[2], v[3]);
    }
}
__device__ __forceinline__ float elem(const void* p, int bf16, long long idx) {
    return bf16 ? dhaug_bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[idx]) : reinterpret_cast<const float*>(p)[idx];
}

// ------------------------------------------------------------------------------------------------------------ LayerNorm
constexpr int kLnBlock = 256;
constexpr int kLnChunks = 8;                               // four-element chunks a lane keeps
constexpr int kLnMaxCols = DHAUG_LAYERNORM_MAX_COLS;
constexpr int kLnMaxBlocks = DHAUG_LAYERNORM_MAX_BLOCKS;
constexpr int kLnRowGrid = 256 * 8;
static_assert(kLnMaxCols == 64 * kLnChunks * 4, "64 lanes x 8 chunks x 4 elements");

struct LnArgs {
    const void* x; const void* g; void* y;                 // forward: x -> y; backward: x, g -> y = dx
    const float* gamma; const float* beta;
    float* mean; float* rstd;                              // forward: written (each may be null); backward: read
    long long ld_x, ld_g, ld_y, M;
    int C, x_bf16, g_bf16, y_bf16;
    float eps;
};

template <int LPR>
__device__ __forceinline__ float row_sum(float s) {
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    return s;
}

template <int LPR, bool BWD>
__global__ __launch_bounds__(kLnBlock) void layernorm_kernel(LnArgs a) {
    constexpr int ROWS = kLnBlock / LPR;
    const int sub = threadIdx.x % LPR, nch = a.C >> 2;
    const float invC = 1.0f / (float)a.C;
    const long long groups = (a.M + ROWS - 1) / ROWS;
    for (long long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long long row = grp * ROWS + threadIdx.x / LPR;
        const bool live = row < a.M;                       // (the lanes of a row are live together: the butterflies stay inside a row)
        float v[kLnChunks][4];
#pragma unroll
        for (int k = 0; k < kLnChunks; ++k) {
            const int ch = sub + k * LPR;
            if (live && ch < nch) load4(a.x, a.x_bf16, row * a.ld_x + 4 * ch, v[k]);
            else v[k][0] = v[k][1] = v[k][2] = v[k][3] = 0.0f;
        }
        if constexpr (!BWD) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < kLnChunks; ++k) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
            const float m0 = row_sum<LPR>(s) * invC;
            float c = 0.0f;
#pragma unroll
            for (int k = 0; k < kLnChunks; ++k)
                if (sub + k * LPR < nch) c += ((v[k][0] - m0) + (v[k][1] - m0)) + ((v[k][2] - m0) + (v[k][3] - m0));
            const float mean = m0 + row_sum<LPR>(c) * invC;
            // what fp32 cannot hold of the mean (half an ulp of it at most) is taken off the centred values themselves
            float r = 0.0f;
#pragma unroll
            for (int k = 0; k < kLnChunks; ++k)
                if (sub + k * LPR < nch) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[k][e] -= mean;
                    r += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
                }
            r = row_sum<LPR>(r) * invC;
            float ss = 0.0f;
#pragma unroll
            for (int k = 0; k < kLnChunks; ++k)
                if (sub + k * LPR < nch) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[k][e] -= r; ss = fmaf(v[k][e], v[k][e], ss); }
                }
            const float rstd = 1.0f / sqrtf(row_sum<LPR>(ss) * invC + a.eps);
            if (live) {
#pragma unroll
                for (int k = 0; k < kLnChunks; ++k) {
                    const int ch = sub + k * LPR;
                    if (ch < nch) {
                        float o[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = v[k][e] * rstd * a.gamma[4 * ch + e] + a.beta[4 * ch + e];
                        store4(a.y, a.y_bf16, row * a.ld_y + 4 * ch, o);
                    }
                }
                if (sub == 0) {
                    if (a.mean != nullptr) a.mean[row] = mean;
                    if (a.rstd != nullptr) a.rstd[row] = rstd;
                }
            }
        } else {
            const float mean = live ? a.mean[row] : 0.0f, rstd = live ? a.rstd[row] : 0.0f;
            float gg[kLnChunks][4];
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < kLnChunks; ++k) {
                const int ch = sub + k * LPR;
                if (live && ch < nch) {
                    load4(a.g, a.g_bf16, row * a.ld_g + 4 * ch, gg[k]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[k][e] = (v[k][e] - mean) * rstd;
                        gg[k][e] *= a.gamma[4 * ch + e];
                        s1 += gg[k][e];
                        s2 = fmaf(gg[k][e], v[k][e], s2);
                    }
                } else {
                    gg[k][0] = gg[k][1] = gg[k][2] = gg[k][3] = 0.0f;
                }
            }
            s1 = row_sum<LPR>(s1) * invC;
            s2 = row_sum<LPR>(s2) * invC;
            if (live) {
#pragma unroll
                for (int k = 0; k < kLnChunks; ++k) {
                    const int ch = sub + k * LPR;
                    if (ch < nch) {
                        float o[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = rstd * ((gg[k][e] - s1) - v[k][e] * s2);
                        store4(a.y, a.y_bf16, row * a.ld_y + 4 * ch, o);
                    }
                }
            }
        }
    }
}

template <bool BWD>
void launch_layernorm(const LnArgs& a, hipStream_t stream) {
    const int lpr = a.C <= 128 ? 4 : (a.C <= 512 ? 16 : 64);
    const unsigned grid = (unsigned)dhaug_stream_grid(a.M, kLnBlock / lpr, kLnRowGrid);
    if (lpr == 4) hipLaunchKernelGGL((layernorm_kernel<4, BWD>), dim3(grid), dim3(kLnBlock), 0, stream, a);
    else if (lpr == 16) hipLaunchKernelGGL((layernorm_kernel<16, BWD>), dim3(grid), dim3(kLnBlock), 0, stream, a);
    else hipLaunchKernelGGL((layernorm_kernel<64, BWD>), dim3(grid), dim3(kLnBlock), 0, stream, a);
}

// dgamma[c] = sum_r g[r,c] xhat[r,c], dbeta[c] = sum_r g[r,c]: workgroup (column tile, row slice); a thread owns one column and every
// lanes-th row of the slice, fp64 sums in row order; the row lanes are added in lane order; ws[(slice * 2 + which) * C + c]
struct LnParamArgs {
    const void* x; const void* g; const float* mean; const float* rstd; double* ws;
    long long ld_x, ld_g, M, rows_per_block;
    int C, x_bf16, g_bf16, tile;                           // tile: columns of a workgroup, 32 or 64
};

__global__ __launch_bounds__(kLnBlock) void layernorm_param_partials_kernel(LnParamArgs a) {
    __shared__ double red[2][kLnBlock];
    const int tx = threadIdx.x % a.tile, ty = threadIdx.x / a.tile, lanes = kLnBlock / a.tile;
    const int c = blockIdx.x * a.tile + tx;
    const long long r0 = (long long)blockIdx.y * a.rows_per_block;
    const long long r1 = r0 + a.rows_per_block < a.M ? r0 + a.rows_per_block : a.M;
    double sg = 0.0, sb = 0.0;
    if (c < a.C)
        for (long long r = r0 + ty; r < r1; r += lanes) {
            const float g = elem(a.g, a.g_bf16, r * a.ld_g + c);
            const float xh = (elem(a.x, a.x_bf16, r * a.ld_x + c) - a.mean[r]) * a.rstd[r];
            sg += (double)g * (double)xh;
            sb += (double)g;
        }
    red[0][threadIdx.x] = sg;
    red[1][threadIdx.x] = sb;
    __syncthreads();
    if (ty == 0 && c < a.C) {
        for (int k = 1; k < lanes; ++k) { sg += red[0][k * a.tile + tx]; sb += red[1][k * a.tile + tx]; }
        double* w = a.ws + (long long)blockIdx.y * 2 * a.C;
        w[c] = sg;
        w[a.C + c] = sb;
    }
}

__global__ __launch_bounds__(256) void layernorm_param_finish_kernel(const double* __restrict__ ws, int blocks, int C,
                                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double sg = 0.0, sb = 0.0;
    for (int b = 0; b < blocks; ++b) { sg += ws[(long long)b * 2 * C + c]; sb += ws[(long long)b * 2 * C + C + c]; }
    dgamma[c] = (float)sg;
    dbeta[c] = (float)sb;
}

// row tensors of the vector kernels: base and pitch on the 4-element grid
inline bool rows_ok(const void* p, int bf16, int64_t ld) { return aligned(p, bf16 ? 8 : 16) && ld % 4 == 0; }
inline bool flag(int v) { return v == 0 || v == 1; }

// ------------------------------------------------------------------------------------------------------------ attention
constexpr int kAttnBlock = 256;
constexpr int kAttnMaxTokens = DHAUG_ATTN_MAX_TOKENS;
constexpr int kAttnMaxHead = DHAUG_ATTN_MAX_HEAD_DIM;
constexpr int kAttnMaxBlocks = DHAUG_ATTN_MAX_BLOCKS;
constexpr int kAttnLds = 64 * 1024;                        // what a workgroup's pairs may take together (one pair may take more)
constexpr int kAttnPairPad = 4;                            // floats between the pairs' K (V) blocks: pairs of a wave on different banks
// the backward kernel's largest single pair: K|V (Q|dO) plus P and dS
constexpr int kAttnBwdMaxLds = (2 * (kAttnMaxTokens * kAttnMaxHead + kAttnPairPad) + 2 * kAttnMaxTokens * (kAttnMaxTokens | 1)) * 4;

struct AttnArgs {
    const void* qkv; const void* dout;                                            // read
    void* out_w; float* lse_w; void* dqkv;                                        // written
    long long ld_qkv, ld_out, ld_dout, ld_dqkv, pairs, groups;
    int N, H, hd, P, pstride;                              // P: pairs of a workgroup; pstride: floats of a pair's K (V) block
    int qkv_bf16, out_bf16, dout_bf16, dqkv_bf16;
    float scale;
};

// rows [0, N) x columns [col0 + h hd, + hd) of the workgroup's pairs from a row tensor into dst[pair][j * hd + d] (fp32)
__device__ __forceinline__ void attn_stage(float* __restrict__ dst, const void* __restrict__ src, int bf16, long long ld, long long col0,
                                           long long pair0, int np, const AttnArgs& a) {
    const int hd4 = a.hd >> 2, per_pair = a.N * hd4, total = np * per_pair;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int pp = idx / per_pair, r = idx - pp * per_pair, j = r / hd4, c = r - j * hd4;
        const long long pair = pair0 + pp, s = pair / a.H, h = pair - s * a.H;
        float v[4];
        load4(src, bf16, (s * a.N + j) * ld + col0 + h * a.hd + 4 * c, v);
        *reinterpret_cast<float4*>(dst + pp * a.pstride + j * a.hd + 4 * c) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

template <int CH>
__device__ __forceinline__ float dot_row(const float (&q)[CH][4], const float* __restrict__ row, int hd4) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (c < hd4) {
            const float4 k = *reinterpret_cast<const float4*>(row + 4 * c);
            s = fmaf(q[c][0], k.x, s); s = fmaf(q[c][1], k.y, s); s = fmaf(q[c][2], k.z, s); s = fmaf(q[c][3], k.w, s);
        }
    return s;
}
template <int CH>
__device__ __forceinline__ void axpy_row(float (&acc)[CH][4], float w, const float* __restrict__ row, int hd4) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (c < hd4) {
            const float4 k = *reinterpret_cast<const float4*>(row + 4 * c);
            acc[c][0] = fmaf(w, k.x, acc[c][0]); acc[c][1] = fmaf(w, k.y, acc[c][1]);
            acc[c][2] = fmaf(w, k.z, acc[c][2]); acc[c][3] = fmaf(w, k.w, acc[c][3]);
        }
}
template <int CH>
__device__ __forceinline__ void load_row(float (&q)[CH][4], const void* p, int bf16, long long idx, int hd4) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        if (c < hd4) load4(p, bf16, idx + 4 * c, q[c]);
        else q[c][0] = q[c][1] = q[c][2] = q[c][3] = 0.0f;
    }
}
template <int CH>
__device__ __forceinline__ void store_row(void* p, int bf16, long long idx, const float (&acc)[CH][4], float w, int hd4) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (c < hd4) {
            const float o[4] = {acc[c][0] * w, acc[c][1] * w, acc[c][2] * w, acc[c][3] * w};
            store4(p, bf16, idx + 4 * c, o);
        }
}

// CH: four-element chunks of a head the lane keeps (hd <= 4 CH)
template <int CH>
__global__ __launch_bounds__(kAttnBlock) void attn_forward_kernel(AttnArgs a) {
    extern __shared__ float4 attn_lds4[];
    float* Ks = reinterpret_cast<float*>(attn_lds4);
    float* Vs = Ks + a.P * a.pstride;
    const int N = a.N, hd = a.hd, hd4 = hd >> 2;
    const long long C = (long long)a.H * hd;
    const int pl = threadIdx.x / N, i = threadIdx.x - pl * N;
    for (long long grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const long long pair0 = grp * a.P;
        const int np = a.pairs - pair0 < a.P ? (int)(a.pairs - pair0) : a.P;
        attn_stage(Ks, a.qkv, a.qkv_bf16, a.ld_qkv, C, pair0, np, a);
        attn_stage(Vs, a.qkv, a.qkv_bf16, a.ld_qkv, 2 * C, pair0, np, a);
        __syncthreads();
        if (pl < np) {
            const long long pair = pair0 + pl, s = pair / a.H, h = pair - s * a.H, row = s * N + i;
            float q[CH][4], acc[CH][4];
            load_row<CH>(q, a.qkv, a.qkv_bf16, row * a.ld_qkv + h * hd, hd4);
            const float* kp = Ks + pl * a.pstride;
            const float* vp = Vs + pl * a.pstride;
            float m = -INFINITY;
            for (int j = 0; j < N; ++j) m = fmaxf(m, dot_row<CH>(q, kp + j * hd, hd4) * a.scale);
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.0f;
            float l = 0.0f;
            for (int j = 0; j < N; ++j) {
                const float p = expf(dot_row<CH>(q, kp + j * hd, hd4) * a.scale - m);
                l += p;
                axpy_row<CH>(acc, p, vp + j * hd, hd4);
            }
            store_row<CH>(a.out_w, a.out_bf16, row * a.ld_out + h * hd, acc, 1.0f / l, hd4);
            if (a.lse_w != nullptr) a.lse_w[pair * N + i] = m + logf(l);
        }
        __syncthreads();
    }
}

template <int CH>
__global__ __launch_bounds__(kAttnBlock) void attn_backward_kernel(AttnArgs a) {
    extern __shared__ float4 attn_lds4[];
    const int N = a.N, NP = N | 1, hd = a.hd, hd4 = hd >> 2;
    float* A0 = reinterpret_cast<float*>(attn_lds4);       // K, then Q
    float* A1 = A0 + a.P * a.pstride;                      // V, then dO
    float* Pm = A1 + a.P * a.pstride;                      // [pair][query][key], rows NP apart (odd: lanes on different banks)
    float* Sm = Pm + a.P * N * NP;
    const long long C = (long long)a.H * hd;
    const int pl = threadIdx.x / N, i = threadIdx.x - pl * N;
    for (long long grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const long long pair0 = grp * a.P;
        const int np = a.pairs - pair0 < a.P ? (int)(a.pairs - pair0) : a.P;
        const long long pair = pair0 + pl, s = pair / a.H, h = pair - s * a.H, row = s * N + i;
        attn_stage(A0, a.qkv, a.qkv_bf16, a.ld_qkv, C, pair0, np, a);
        attn_stage(A1, a.qkv, a.qkv_bf16, a.ld_qkv, 2 * C, pair0, np, a);
        __syncthreads();
        if (pl < np) {                                     // phase 1: lane = query i
            float q[CH][4], go[CH][4], acc[CH][4];
            load_row<CH>(q, a.qkv, a.qkv_bf16, row * a.ld_qkv + h * hd, hd4);
            load_row<CH>(go, a.dout, a.dout_bf16, row * a.ld_dout + h * hd, hd4);
            const float* kp = A0 + pl * a.pstride;
            const float* vp = A1 + pl * a.pstride;
            float* prow = Pm + (pl * N + i) * NP;
            float* srow = Sm + (pl * N + i) * NP;
            // P as the forward pass formed it, bit for bit: the same scores in the same order, their maximum, exp and the sum again
            // (exp(score - lse) would carry the rounding of lse, half an ulp of a number the size of the largest score, into every
            // weight: 4e-6 at scores of 80).  The scores wait in the row of LDS that P takes.
            float m = -INFINITY;
            for (int j = 0; j < N; ++j) {
                const float sc = dot_row<CH>(q, kp + j * hd, hd4) * a.scale;
                prow[j] = sc;
                m = fmaxf(m, sc);
            }
            float l = 0.0f;
            for (int j = 0; j < N; ++j) {
                const float p = expf(prow[j] - m);
                l += p;
                prow[j] = p;
                srow[j] = dot_row<CH>(go, vp + j * hd, hd4);
            }
            // D_i = sum_j P_ij dP_ij from the same dP that dS uses (not dout . out): where P is peaked, dP_ij - D_i then cancels the
            // rounding of dP_ij itself, as in torch's softmax backward
            const float inv = 1.0f / l;
            float D = 0.0f;
            for (int j = 0; j < N; ++j) {
                const float p = prow[j] * inv;
                prow[j] = p;
                D = fmaf(p, srow[j], D);
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.0f;
            for (int j = 0; j < N; ++j) {
                const float ds = prow[j] * (srow[j] - D);
                srow[j] = ds;
                axpy_row<CH>(acc, ds, kp + j * hd, hd4);
            }
            store_row<CH>(a.dqkv, a.dqkv_bf16, row * a.ld_dqkv + h * hd, acc, a.scale, hd4);
        }
        __syncthreads();
        attn_stage(A0, a.qkv, a.qkv_bf16, a.ld_qkv, 0, pair0, np, a);
        attn_stage(A1, a.dout, a.dout_bf16, a.ld_dout, 0, pair0, np, a);
        __syncthreads();
        if (pl < np) {                                     // phase 2: lane = key i
            float dk[CH][4], dv[CH][4];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                dk[c][0] = dk[c][1] = dk[c][2] = dk[c][3] = 0.0f;
                dv[c][0] = dv[c][1] = dv[c][2] = dv[c][3] = 0.0f;
            }
            const float* qp = A0 + pl * a.pstride;
            const float* gp = A1 + pl * a.pstride;
            const float* pcol = Pm + pl * N * NP + i;
            const float* scol = Sm + pl * N * NP + i;
            for (int r = 0; r < N; ++r) {
                axpy_row<CH>(dv, pcol[r * NP], gp + r * hd, hd4);
                axpy_row<CH>(dk, scol[r * NP], qp + r * hd, hd4);
            }
            store_row<CH>(a.dqkv, a.dqkv_bf16, row * a.ld_dqkv + C + h * hd, dk, a.scale, hd4);
            store_row<CH>(a.dqkv, a.dqkv_bf16, row * a.ld_dqkv + 2 * C + h * hd, dv, 1.0f, hd4);
        }
        __syncthreads();
    }
}

// pairs of a workgroup: as many as 256 lanes and the LDS budget hold, at least one
inline int attn_pairs(int N, int pair_bytes) {
    int P = kAttnBlock / N;
    const int fit = kAttnLds / pair_bytes;
    if (P > fit) P = fit;
    return P < 1 ? 1 : P;
}

int attn_check(int64_t S, int N, int H, int hd) {
    DHAUG_CHECK(S >= 0 && N >= 0 && H >= 0 && hd >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(N >= 1 && N <= kAttnMaxTokens && hd >= 4 && hd <= kAttnMaxHead && hd % 4 == 0, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(H < (1 << 20) && S < kMaxRows / kAttnMaxTokens, DHAUG_EUNSUPPORTED);
    return DHAUG_OK;
}

template <template <int> class L>
int attn_dispatch(int hd, const AttnArgs& a, unsigned grid, unsigned block, int lds, hipStream_t stream) {
    const int hd4 = hd >> 2;
    if (hd4 <= 1) return L<1>::run(a, grid, block, lds, stream);
    if (hd4 <= 2) return L<2>::run(a, grid, block, lds, stream);
    if (hd4 <= 4) return L<4>::run(a, grid, block, lds, stream);
    if (hd4 <= 8) return L<8>::run(a, grid, block, lds, stream);
    return L<16>::run(a, grid, block, lds, stream);
}
template <int CH> struct FwdLaunch {
    static int run(const AttnArgs& a, unsigned grid, unsigned block, int lds, hipStream_t stream) {
        hipLaunchKernelGGL(attn_forward_kernel<CH>, dim3(grid), dim3(block), lds, stream, a);
        return dhaug_launch_status();
    }
};
template <int CH> struct BwdLaunch {
    static int run(const AttnArgs& a, unsigned grid, unsigned block, int lds, hipStream_t stream) {
        if (const int rc = dhaug_dynamic_lds<attn_backward_kernel<CH>>(kAttnBwdMaxLds)) return rc;
        hipLaunchKernelGGL(attn_backward_kernel<CH>, dim3(grid), dim3(block), lds, stream, a);
        return dhaug_launch_status();
    }
};

// ------------------------------------------------------------------------------------------------------------ GELU
constexpr int kGeluBlock = 256;
constexpr int kGeluMaxBlocks = DHAUG_GELU_MAX_BLOCKS;

struct GeluArgs {
    const float* z; const void* g; void* y;
    long long ld_z, ld_g, ld_y, M;
    int C, g_bf16, y_bf16;
};

__device__ __forceinline__ float gelu_cdf(float z) { return 0.5f * erfcf(-z * 0.70710678118654752440f); }

template <bool BWD>
__global__ __launch_bounds__(kGeluBlock) void gelu_kernel(GeluArgs a) {
    const long long nv = a.C >> 2, items = a.M * nv, stride = (long long)gridDim.x * kGeluBlock;
    for (long long it = (long long)blockIdx.x * kGeluBlock + threadIdx.x; it < items; it += stride) {
        const long long r = it / nv, col = (it - r * nv) * 4;
        float z[4], o[4];
        load4(a.z, 0, r * a.ld_z + col, z);
        if (BWD) {
            float g[4];
            load4(a.g, a.g_bf16, r * a.ld_g + col, g);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = g[e] * (gelu_cdf(z[e]) + z[e] * (0.39894228040143267794f * expf(-0.5f * z[e] * z[e])));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = z[e] * gelu_cdf(z[e]);
        }
        store4(a.y, a.y_bf16, r * a.ld_y + col, o);
    }
    // the columns behind the last whole vector (C % 4 of them), element by element
    const int tail = a.C & 3;
    if (tail) {
        const long long c0 = a.C - tail, titems = a.M * tail;
        for (long long it = (long long)blockIdx.x * kGeluBlock + threadIdx.x; it < titems; it += stride) {
            const long long r = it / tail, col = c0 + (it - r * tail);
            const float z = a.z[r * a.ld_z + col];
            float o;
            if (BWD) o = elem(a.g, a.g_bf16, r * a.ld_g + col) * (gelu_cdf(z) + z * (0.39894228040143267794f * expf(-0.5f * z * z)));
            else o = z * gelu_cdf(z);
            if (a.y_bf16) reinterpret_cast<uint16_t*>(a.y)[r * a.ld_y + col] = dhaug_f32_to_bf16(o);
            else reinterpret_cast<float*>(a.y)[r * a.ld_y + col] = o;
        }
    }
}

}  // namespace

extern "C" int dhaug_layernorm_forward(const void* x, int x_bf16, int64_t ld_x, const float* gamma, const float* beta, float eps,
                                       void* y, int y_bf16, int64_t ld_y, float* mean, float* rstd, int64_t M, int64_t C, void* stream) {
    DHAUG_CHECK(M >= 0 && C >= 0 && flag(x_bf16) && flag(y_bf16) && eps >= 0.0f, DHAUG_EINVAL);
    if (M == 0 || C == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(x); DHAUG_CHECK_PTR(gamma); DHAUG_CHECK_PTR(beta); DHAUG_CHECK_PTR(y);
    DHAUG_CHECK(C % 16 == 0 && C <= kLnMaxCols && M < kMaxRows, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(ld_x >= C && ld_y >= C && rows_ok(x, x_bf16, ld_x) && rows_ok(y, y_bf16, ld_y), DHAUG_EALIGN);
    DHAUG_CHECK(aligned(gamma, 4) && aligned(beta, 4) && aligned(mean, 4) && aligned(rstd, 4), DHAUG_EALIGN);
    LnArgs a = {};
    a.x = x; a.y = y; a.gamma = gamma; a.beta = beta; a.mean = mean; a.rstd = rstd; a.ld_x = ld_x; a.ld_y = ld_y; a.M = M;
    a.C = (int)C; a.x_bf16 = x_bf16; a.y_bf16 = y_bf16; a.eps = eps;
    launch_layernorm<false>(a, (hipStream_t)stream);
    return dhaug_launch_status();
}

extern "C" int dhaug_layernorm_backward(const void* x, int x_bf16, int64_t ld_x, const void* g, int g_bf16, int64_t ld_g,
                                        const float* gamma, const float* mean, const float* rstd, void* dx, int dx_bf16,
                                        int64_t ld_dx, float* dgamma, float* dbeta, void* workspace, int64_t M, int64_t C,
                                        void* stream) {
    DHAUG_CHECK(M >= 0 && C >= 0 && flag(x_bf16) && flag(g_bf16) && flag(dx_bf16), DHAUG_EINVAL);
    DHAUG_CHECK((dgamma == nullptr) == (dbeta == nullptr) && (dx != nullptr || dgamma != nullptr), DHAUG_EINVAL);
    if (C == 0) return DHAUG_OK;
    DHAUG_CHECK(C % 16 == 0 && C <= kLnMaxCols && M < kMaxRows, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(aligned(dgamma, 4) && aligned(dbeta, 4) && aligned(workspace, 8), DHAUG_EALIGN);
    if (M > 0) {                                           // (every check in front of the first launch)
        DHAUG_CHECK_PTR(x); DHAUG_CHECK_PTR(g); DHAUG_CHECK_PTR(mean); DHAUG_CHECK_PTR(rstd);
        if (dx != nullptr) DHAUG_CHECK_PTR(gamma);
        if (dgamma != nullptr) DHAUG_CHECK_PTR(workspace);
        DHAUG_CHECK(ld_x >= C && ld_g >= C && rows_ok(x, x_bf16, ld_x) && rows_ok(g, g_bf16, ld_g), DHAUG_EALIGN);
        DHAUG_CHECK(aligned(mean, 4) && aligned(rstd, 4), DHAUG_EALIGN);
        DHAUG_CHECK(dx == nullptr || (ld_dx >= C && rows_ok(dx, dx_bf16, ld_dx) && aligned(gamma, 4)), DHAUG_EALIGN);
    }
    if (dx != nullptr && M > 0) {
        LnArgs a = {};
        a.x = x; a.g = g; a.y = dx; a.gamma = gamma; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd);
        a.ld_x = ld_x; a.ld_g = ld_g; a.ld_y = ld_dx; a.M = M; a.C = (int)C; a.x_bf16 = x_bf16; a.g_bf16 = g_bf16; a.y_bf16 = dx_bf16;
        launch_layernorm<true>(a, (hipStream_t)stream);
        const int rc = dhaug_launch_status();
        if (rc != DHAUG_OK) return rc;
    }
    if (dgamma != nullptr) {
        int blocks = 0;
        if (M > 0) {
            LnParamArgs p = {};
            p.x = x; p.g = g; p.mean = mean; p.rstd = rstd; p.ws = (double*)workspace; p.ld_x = ld_x; p.ld_g = ld_g; p.M = M;
            p.C = (int)C; p.x_bf16 = x_bf16; p.g_bf16 = g_bf16; p.tile = C <= 32 ? 32 : 64;
            const int64_t lanes = kLnBlock / p.tile, want = (M + lanes - 1) / lanes < kLnMaxBlocks ? (M + lanes - 1) / lanes : kLnMaxBlocks;
            p.rows_per_block = (M + want - 1) / want;
            blocks = (int)((M + p.rows_per_block - 1) / p.rows_per_block);
            hipLaunchKernelGGL(layernorm_param_partials_kernel, dim3((unsigned)((C + p.tile - 1) / p.tile), (unsigned)blocks), dim3(kLnBlock),
                               0, (hipStream_t)stream, p);
            const int rc = dhaug_launch_status();
            if (rc != DHAUG_OK) return rc;
        }
        hipLaunchKernelGGL(layernorm_param_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const double*)workspace, blocks, (int)C, dgamma, dbeta);
    }
    return dhaug_launch_status();
}

extern "C" int dhaug_attn_forward(const void* qkv, int qkv_bf16, int64_t ld_qkv, void* out, int out_bf16, int64_t ld_out, float* lse,
                                  int64_t S, int N, int H, int hd, float scale, void* stream) {
    DHAUG_CHECK(flag(qkv_bf16) && flag(out_bf16), DHAUG_EINVAL);
    if (const int rc = attn_check(S, N, H, hd)) return rc;
    if (S == 0 || H == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(qkv); DHAUG_CHECK_PTR(out);
    const int64_t C = (int64_t)H * hd;
    DHAUG_CHECK(ld_qkv >= 3 * C && ld_out >= C && rows_ok(qkv, qkv_bf16, ld_qkv) && rows_ok(out, out_bf16, ld_out) && aligned(lse, 4),
                DHAUG_EALIGN);
    AttnArgs a = {};
    a.qkv = qkv; a.out_w = out; a.lse_w = lse; a.ld_qkv = ld_qkv; a.ld_out = ld_out; a.pairs = S * H; a.N = N; a.H = H; a.hd = hd;
    a.pstride = N * hd + kAttnPairPad;
    a.P = attn_pairs(N, 2 * a.pstride * 4);
    a.groups = (a.pairs + a.P - 1) / a.P;
    a.qkv_bf16 = qkv_bf16; a.out_bf16 = out_bf16; a.scale = scale;
    const unsigned block = (unsigned)((a.P * N + 63) / 64 * 64);
    const unsigned grid = (unsigned)(a.groups < kAttnMaxBlocks ? a.groups : kAttnMaxBlocks);
    return attn_dispatch<FwdLaunch>(hd, a, grid, block, a.P * 2 * a.pstride * 4, (hipStream_t)stream);
}

extern "C" int dhaug_attn_backward(const void* qkv, int qkv_bf16, int64_t ld_qkv, const void* out, int out_bf16, int64_t ld_out,
                                   const float* lse, const void* dout, int dout_bf16, int64_t ld_dout, void* dqkv, int dqkv_bf16,
                                   int64_t ld_dqkv, int64_t S, int N, int H, int hd, float scale, void* stream) {
    DHAUG_CHECK(flag(qkv_bf16) && flag(out_bf16) && flag(dout_bf16) && flag(dqkv_bf16), DHAUG_EINVAL);
    if (const int rc = attn_check(S, N, H, hd)) return rc;
    if (S == 0 || H == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(qkv); DHAUG_CHECK_PTR(out); DHAUG_CHECK_PTR(lse); DHAUG_CHECK_PTR(dout); DHAUG_CHECK_PTR(dqkv);
    DHAUG_CHECK(qkv != dqkv, DHAUG_EINVAL);
    const int64_t C = (int64_t)H * hd;
    DHAUG_CHECK(ld_qkv >= 3 * C && ld_out >= C && ld_dout >= C && ld_dqkv >= 3 * C, DHAUG_EALIGN);
    DHAUG_CHECK(rows_ok(qkv, qkv_bf16, ld_qkv) && rows_ok(out, out_bf16, ld_out) && rows_ok(dout, dout_bf16, ld_dout) &&
                rows_ok(dqkv, dqkv_bf16, ld_dqkv) && aligned(lse, 4), DHAUG_EALIGN);
    AttnArgs a = {};
    a.qkv = qkv; a.dout = dout; a.dqkv = dqkv;            // (out and lse: checked above, not read -- see include/dhaug.h)
    a.ld_qkv = ld_qkv; a.ld_out = ld_out; a.ld_dout = ld_dout;
    a.ld_dqkv = ld_dqkv; a.pairs = S * H; a.N = N; a.H = H; a.hd = hd;
    a.pstride = N * hd + kAttnPairPad;
    const int pair_bytes = (2 * a.pstride + 2 * N * (N | 1)) * 4;
    a.P = attn_pairs(N, pair_bytes);
    a.groups = (a.pairs + a.P - 1) / a.P;
    a.qkv_bf16 = qkv_bf16; a.out_bf16 = out_bf16; a.dout_bf16 = dout_bf16; a.dqkv_bf16 = dqkv_bf16; a.scale = scale;
    const unsigned block = (unsigned)((a.P * N + 63) / 64 * 64);
    const unsigned grid = (unsigned)(a.groups < kAttnMaxBlocks ? a.groups : kAttnMaxBlocks);
    return attn_dispatch<BwdLaunch>(hd, a, grid, block, a.P * pair_bytes, (hipStream_t)stream);
}

static int gelu_launch(const float* z, int64_t ld_z, const void* g, int g_bf16, int64_t ld_g, void* y, int y_bf16, int64_t ld_y,
                       int64_t M, int64_t C, bool bwd, void* stream) {
    DHAUG_CHECK(M >= 0 && C >= 0 && flag(g_bf16) && flag(y_bf16), DHAUG_EINVAL);
    if (M == 0 || C == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(z); DHAUG_CHECK_PTR(y);
    if (bwd) DHAUG_CHECK_PTR(g);
    DHAUG_CHECK(C < (1ll << 28) && M < kMaxRows, DHAUG_EUNSUPPORTED);
    // (a single row has no pitch to keep on the vector grid)
    DHAUG_CHECK(ld_z >= C && ld_y >= C && rows_ok(z, 0, M == 1 ? 0 : ld_z) && rows_ok(y, y_bf16, M == 1 ? 0 : ld_y), DHAUG_EALIGN);
    DHAUG_CHECK(!bwd || (ld_g >= C && rows_ok(g, g_bf16, M == 1 ? 0 : ld_g)), DHAUG_EALIGN);
    GeluArgs a = {};
    a.z = z; a.g = g; a.y = y; a.ld_z = ld_z; a.ld_g = ld_g; a.ld_y = ld_y; a.M = M; a.C = (int)C; a.g_bf16 = g_bf16; a.y_bf16 = y_bf16;
    const unsigned grid = (unsigned)dhaug_stream_grid(M * ((C + 3) / 4), kGeluBlock, kGeluMaxBlocks);
    if (bwd) hipLaunchKernelGGL(gelu_kernel<true>, dim3(grid), dim3(kGeluBlock), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gelu_kernel<false>, dim3(grid), dim3(kGeluBlock), 0, (hipStream_t)stream, a);
    return dhaug_launch_status();
}

extern "C" int dhaug_gelu_forward(const float* z, int64_t ld_z, void* y, int y_bf16, int64_t ld_y, int64_t M, int64_t C, void* stream) {
    return gelu_launch(z, ld_z, nullptr, 0, 0, y, y_bf16, ld_y, M, C, false, stream);
}

extern "C" int dhaug_gelu_backward(const float* z, int64_t ld_z, const void* g, int g_bf16, int64_t ld_g, void* dz, int dz_bf16,
                                   int64_t ld_dz, int64_t M, int64_t C, void* stream) {
    return gelu_launch(z, ld_z, g, g_bf16, ld_g, dz, dz_bf16, ld_dz, M, C, true, stream);
}
