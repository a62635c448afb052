// The layer of the single-frame VideoPose posenet between two GEMMs (R/models_baseline/videopose/model_VideoPose3D.py:163-220:
// BatchNorm1d in training mode -> ReLU -> Dropout (+ the block's residual)), forward and backward, and the evaluation-mode fold of
// a BatchNorm into the convolution in front of it.  The convolutions themselves (kernel width 1 on a length-1 sequence: dense
// layers) are dhaug_gemm_bf16 / the split-operand GEMMs.
//
//  dhaug_bn_partials               per (column strip, row chunk): sum z and sum z^2 per column in fp64 (products of fp32 values are exact
//                                  in fp64: no Welford, no shift) -> workspace (chunks, 2, C).
//  dhaug_bn_act_forward            prologue: the strip's columns add their chunk partials in chunk order (the launch-boundary reduce of
//                                  dhaug_adam_clip_step: no third launch) -> mean, biased var, rstd; then
//                                  y = keep * relu((z - mean) * rstd * gamma + beta) / (1 - p) (+ residual).  Row chunk 0 keeps mean / rstd
//                                  for the backward pass and updates running_mean / running_var / num_batches_tracked as nn.BatchNorm1d.
//  dhaug_bn_act_backward_partials  gz = g * keep / (1 - p) * [pre-activation > 0]: sum gz and sum gz * xhat per column and chunk, fp64.
//  dhaug_bn_act_backward           dz = gamma * rstd * (gz - sum gz / M - xhat * sum(gz xhat) / M); chunk 0 writes dgamma, dbeta.
//  dhaug_bn_act_forward_dr, dhaug_bn_act_backward_partials_dr, dhaug_bn_act_backward_dr
//                                  the three kernels above instantiated with DR = true: (seed, offset) = (cell[0], cell[1] + delta) read from
//                                  device memory, so a launch captured in a hipGraph draws a new mask at every replay.
//  dhaug_bn_fold                   W' = gamma * rstd_run (.) rows of W, b' = beta - running_mean * gamma * rstd_run.
//  dhaug_bn_fold_bias              the same for a layer with a bias b of its own (R/models_baseline/mlp/linear_model.py: nn.Linear in
//                                  front of every BatchNorm): b' = beta + (b - running_mean) * gamma * rstd_run.
//
// No mask is stored: the backward kernels recompute the pre-activation with the forward kernel's own function (bn_pre, below: one
// rounding sequence, nothing for the compiler to contract differently) and regenerate the keep decision from (seed, offset).
// Thread layout of the four training kernels: 8 lanes x 16 bytes cover one 128-byte row segment (32 fp32 / 64 bf16 columns: the strip),
// a workgroup of 256 threads covers 32 rows per pass.  No atomics: the same call gives the same bits.  IEEE semantics (no
// fast-math flag on this file).  NaN convention of these kernels: a NaN pre-activation stays a NaN in y; in the backward pass the test
// is (pre > 0), which a NaN fails, so gz is 0 there.
#include "dhaug_common.h"

#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kLanesPerRow = 8;                           // x 16 bytes = one 128-byte row segment
constexpr int kRowsPerPass = kBlock / kLanesPerRow;       // 32
constexpr int kMaxChunks = DHAUG_BN_MAX_CHUNKS;

template <typename T> struct VecOf;
template <> struct VecOf<float> { static constexpr int N = 4; };
template <> struct VecOf<uint16_t> { static constexpr int N = 8; };

// N elements of a row from column col on; columns at and beyond C are not read (zero)
__device__ __forceinline__ void load_row(const float* __restrict__ p, long long col, long long C, float (&v)[4]) {
    if (col + 4 <= C) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = col + j < C ? p[j] : 0.0f;
    }
}
__device__ __forceinline__ void load_row(const uint16_t* __restrict__ p, long long col, long long C, float (&v)[8]) {
    if (col + 8 <= C) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __builtin_bit_cast(float, w[j] << 16);
            v[2 * j + 1] = __builtin_bit_cast(float, w[j] & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = col + j < C ? dhaug_bf16_to_f32(p[j]) : 0.0f;
    }
}
__device__ __forceinline__ void store_f32(float* __restrict__ p, long long col, long long C, const float (&v)[4]) {
    if (col + 4 <= C) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col + j < C) p[j] = v[j];
    }
}
__device__ __forceinline__ void store_f32(float* __restrict__ p, long long col, long long C, const float (&v)[8]) {
    if (col + 8 <= C) {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (col + j < C) p[j] = v[j];
    }
}
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    return (unsigned)dhaug_f32_to_bf16(lo) | ((unsigned)dhaug_f32_to_bf16(hi) << 16);
}
// bf16 row of the padded operand: columns [C, Cp) are written as zeros, nothing at or beyond Cp (Cp a multiple of 16, col of N)
__device__ __forceinline__ void store_bf16(uint16_t* __restrict__ p, long long col, long long C, const float (&v)[4]) {
    if (col + 4 <= C) {
        *reinterpret_cast<uint2*>(p) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = col + j < C ? dhaug_f32_to_bf16(v[j]) : (uint16_t)0;
    }
}
__device__ __forceinline__ void store_bf16(uint16_t* __restrict__ p, long long col, long long C, const float (&v)[8]) {
    if (col + 8 <= C) {
        *reinterpret_cast<uint4*>(p) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = col + j < C ? dhaug_f32_to_bf16(v[j]) : (uint16_t)0;
    }
}

// Philox4x32-10 (Salmon et al., SC'11) as in dhaug_fk.hip: key = seed, 4 x 32 random bits per call
__device__ __forceinline__ void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                           unsigned (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

struct Drop {
    unsigned long long seed, offset;
    unsigned thresh;            // (uint32)(p * 2^32); 0: no dropout, no random numbers
    float inv_keep;             // 1 / (1 - p)
    const unsigned long long* cell;   // the _dr entries: device words {seed, base}; `offset` then holds the call's delta
};

// The stream position of this launch.  DR = false: the immediates of the launch.  DR = true (the _dr entries, replayable in a captured
// graph): seed = cell[0], offset = cell[1] + delta, a full 64-bit sum; the cell is not read where there is no dropout.
template <bool DR>
__device__ __forceinline__ Drop drop_here(const Drop& d) {
    Drop o = d;
    if (DR && d.thresh) {
        o.seed = d.cell[0];
        o.offset = d.cell[1] + d.offset;
    }
    return o;
}

// keep decisions of the N elements (row, col ..): counter = (element index / 4, offset), element index = row * C + col; the four words
// of one call decide four consecutive elements; keep iff word >= thresh
template <int N>
__device__ __forceinline__ void keep_mask(const Drop& d, long long row, long long col, long long C, bool (&keep)[N]) {
    const unsigned long long e0 = (unsigned long long)row * (unsigned long long)C + (unsigned long long)col;
    unsigned r[4];
    if ((C & 3) == 0) {                                   // (uniform) col is a multiple of 4: whole calls
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const unsigned long long i4 = (e0 >> 2) + q;
            philox4x32((unsigned)i4, (unsigned)(i4 >> 32), (unsigned)d.offset, (unsigned)(d.offset >> 32), (unsigned)d.seed,
                       (unsigned)(d.seed >> 32), r);
#pragma unroll
            for (int j = 0; j < 4; ++j) keep[4 * q + j] = r[j] >= d.thresh;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const unsigned long long e = e0 + j, i4 = e >> 2;
            philox4x32((unsigned)i4, (unsigned)(i4 >> 32), (unsigned)d.offset, (unsigned)(d.offset >> 32), (unsigned)d.seed,
                       (unsigned)(d.seed >> 32), r);
            const unsigned k = (unsigned)(e & 3);
            const unsigned w = k == 0 ? r[0] : (k == 1 ? r[1] : (k == 2 ? r[2] : r[3]));
            keep[j] = w >= d.thresh;
        }
    }
}

// THE pre-activation, shared by the forward and the two backward kernels: xhat = fl((z - mean) * rstd), pre = fma(xhat, gamma, beta).
// A subtraction feeding a multiplication and an explicit fma: -ffp-contract has nothing to decide here.
__device__ __forceinline__ float bn_pre(float z, float mean, float rstd, float gamma, float beta, float& xhat) {
    xhat = (z - mean) * rstd;
    return fmaf(xhat, gamma, beta);
}

struct Common {
    const void* z;
    long long ld_z;
    const float* gamma;
    const float* beta;
    long long M, C, rows_per_chunk;
    int chunks;
    Drop drop;
};

struct FwdArgs {
    Common c;
    const void* res;
    long long ld_res;
    float* mean;                // given statistics: read; otherwise written by row chunk 0
    float* rstd;
    const double* ws;           // null: given statistics
    float* running_mean;
    float* running_var;
    long long* nbt;
    float momentum, eps;
    uint16_t* yb;
    long long ld_yb;
    float* yf;
    long long ld_yf;
};

struct BwdArgs {
    Common c;
    const void* g;
    long long ld_g;
    const float* mean;
    const float* rstd;
    double* ws;                 // partials: written by the first launch, read by the second
    uint16_t* dzb;
    long long ld_dzb;
    float* dzf;
    long long ld_dzf;
    float* dgamma;
    float* dbeta;
};

template <int N>
__device__ __forceinline__ void wave_rows_sum(double (&s)[N]) {
    // lanes with equal (lane & 7) hold the same columns: add the wave's 8 rows
#pragma unroll
    for (int j = 0; j < N; ++j) {
        s[j] += __shfl_xor(s[j], 8);
        s[j] += __shfl_xor(s[j], 16);
        s[j] += __shfl_xor(s[j], 32);
    }
}

// two per-column sums of this workgroup's rows -> ws[(chunk, 0 | 1, column)]: the 8 rows of a wave by butterfly, the four waves in order
template <int N>
__device__ __forceinline__ void write_partials(double (&s)[N], double (&q)[N], double (*lds)[kLanesPerRow][2 * N], long long col,
                                               long long C, double* __restrict__ ws) {
    wave_rows_sum<N>(s);
    wave_rows_sum<N>(q);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < kLanesPerRow) {
#pragma unroll
        for (int j = 0; j < N; ++j) { lds[wave][lane][j] = s[j]; lds[wave][lane][N + j] = q[j]; }
    }
    __syncthreads();
    if (threadIdx.x < kLanesPerRow) {
        double* o = ws + (long long)blockIdx.y * 2 * C;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (col + j < C) {
                o[col + j] = ((lds[0][lane][j] + lds[1][lane][j]) + lds[2][lane][j]) + lds[3][lane][j];
                o[C + col + j] = ((lds[0][lane][N + j] + lds[1][lane][N + j]) + lds[2][lane][N + j]) + lds[3][lane][N + j];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void bn_partials_kernel(const T* __restrict__ z, long long ld, long long M, long long C,
                                                             long long rows_per_chunk, double* __restrict__ ws) {
    constexpr int N = VecOf<T>::N;
    __shared__ double lds[4][kLanesPerRow][2 * N];
    const long long col = ((long long)blockIdx.x * kLanesPerRow + (threadIdx.x & 7)) * N;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk;
    const long long r1 = r0 + rows_per_chunk < M ? r0 + rows_per_chunk : M;
    double s[N], q[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = q[j] = 0.0;
    if (col < C) {
        for (long long r = r0 + (threadIdx.x >> 3); r < r1; r += kRowsPerPass) {
            float v[N];
            load_row(z + r * ld + col, col, C, v);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double d = (double)v[j];
                s[j] += d;
                q[j] += d * d;
            }
        }
    }
    write_partials<N>(s, q, lds, col, C, ws);
}

// the strip's per-column constants in LDS
template <int SC>
struct ColConst {
    float mean[SC], rstd[SC], gamma[SC], beta[SC];
};

template <typename T, bool DR>
__global__ __launch_bounds__(kBlock) void bn_act_forward_kernel(FwdArgs a) {
    constexpr int N = VecOf<T>::N, SC = kLanesPerRow * N;
    __shared__ ColConst<SC> cc;
    const long long M = a.c.M, C = a.c.C, c0 = (long long)blockIdx.x * SC;
    if (threadIdx.x < SC) {
        const long long c = c0 + threadIdx.x;
        float mean = 0.0f, rstd = 0.0f, gm = 0.0f, bt = 0.0f;
        if (c < C) {
            gm = a.c.gamma[c];
            bt = a.c.beta[c];
            if (a.ws == nullptr) {
                mean = a.mean[c];
                rstd = a.rstd[c];
            } else {
                double s = 0.0, q = 0.0;
                for (int k = 0; k < a.c.chunks; ++k) {
                    s += a.ws[(long long)k * 2 * C + c];
                    q += a.ws[(long long)k * 2 * C + C + c];
                }
                const double mu = s / (double)M;
                double var = q / (double)M - mu * mu;
                var = var < 0.0 ? 0.0 : var;                            // (cancellation on a constant column; a NaN stays a NaN)
                mean = (float)mu;
                rstd = (float)(1.0 / sqrt(var + (double)a.eps));
                if (blockIdx.y == 0) {
                    a.mean[c] = mean;
                    a.rstd[c] = rstd;
                    if (a.running_mean) {
                        const float m = a.momentum;
                        const float unbiased = (float)(var * ((double)M / (double)(M - 1)));
                        a.running_mean[c] = (1.0f - m) * a.running_mean[c] + m * mean;
                        a.running_var[c] = (1.0f - m) * a.running_var[c] + m * unbiased;
                    }
                }
            }
        }
        cc.mean[threadIdx.x] = mean; cc.rstd[threadIdx.x] = rstd; cc.gamma[threadIdx.x] = gm; cc.beta[threadIdx.x] = bt;
    }
    if (a.ws != nullptr && a.nbt != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.nbt += 1;
    __syncthreads();

    const int lc = (threadIdx.x & 7) * N;
    const long long col = c0 + lc;
    const long long Cp = (C + 15) / 16 * 16;
    const long long r0 = (long long)blockIdx.y * a.c.rows_per_chunk;
    const long long r1 = r0 + a.c.rows_per_chunk < M ? r0 + a.c.rows_per_chunk : M;
    if (col >= Cp) return;
    const T* z = reinterpret_cast<const T*>(a.c.z);
    const T* res = reinterpret_cast<const T*>(a.res);
    const Drop d = drop_here<DR>(a.c.drop);
    for (long long r = r0 + (threadIdx.x >> 3); r < r1; r += kRowsPerPass) {
        float y[N];
        if (col < C) {
            float v[N], rs[N];
            bool keep[N];
            load_row(z + r * a.c.ld_z + col, col, C, v);
            if (res) load_row(res + r * a.ld_res + col, col, C, rs);
            if (d.thresh) keep_mask<N>(d, r, col, C, keep);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float xh;
                const float pre = bn_pre(v[j], cc.mean[lc + j], cc.rstd[lc + j], cc.gamma[lc + j], cc.beta[lc + j], xh);
                float t = (pre > 0.0f || pre != pre) ? pre : 0.0f;
                if (d.thresh) t = keep[j] ? t * d.inv_keep : 0.0f;
                y[j] = res ? t + rs[j] : t;
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) y[j] = 0.0f;
        }
        if (a.yb) store_bf16(a.yb + r * a.ld_yb + col, col, C, y);
        if (a.yf && col < C) store_f32(a.yf + r * a.ld_yf + col, col, C, y);
    }
}

// gz of one vector: g * keep / (1 - p) where the pre-activation is > 0, else exactly 0; xhat alongside
template <typename T, int N>
__device__ __forceinline__ void gz_of_row(const Common& c, const Drop& d, const T* __restrict__ g, long long ld_g, const float* mean, const float* rstd,
                                          const float* gamma, const float* beta, long long r, long long col, float (&gz)[N],
                                          float (&xh)[N]) {
    float v[N], gv[N];
    bool keep[N];
    load_row(reinterpret_cast<const T*>(c.z) + r * c.ld_z + col, col, c.C, v);
    load_row(g + r * ld_g + col, col, c.C, gv);
    if (d.thresh) keep_mask<N>(d, r, col, c.C, keep);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float pre = bn_pre(v[j], mean[j], rstd[j], gamma[j], beta[j], xh[j]);
        float t = pre > 0.0f ? gv[j] : 0.0f;
        if (d.thresh) t = keep[j] ? t * d.inv_keep : 0.0f;
        gz[j] = t;
    }
}

template <typename T, bool DR>
__global__ __launch_bounds__(kBlock) void bn_act_backward_partials_kernel(BwdArgs a) {
    constexpr int N = VecOf<T>::N, SC = kLanesPerRow * N;
    __shared__ ColConst<SC> cc;
    __shared__ double lds[4][kLanesPerRow][2 * N];
    const long long M = a.c.M, C = a.c.C, c0 = (long long)blockIdx.x * SC;
    if (threadIdx.x < SC) {
        const long long c = c0 + threadIdx.x;
        const bool in = c < C;
        cc.mean[threadIdx.x] = in ? a.mean[c] : 0.0f; cc.rstd[threadIdx.x] = in ? a.rstd[c] : 0.0f;
        cc.gamma[threadIdx.x] = in ? a.c.gamma[c] : 0.0f; cc.beta[threadIdx.x] = in ? a.c.beta[c] : 0.0f;
    }
    __syncthreads();
    const int lc = (threadIdx.x & 7) * N;
    const long long col = c0 + lc;
    const long long r0 = (long long)blockIdx.y * a.c.rows_per_chunk;
    const long long r1 = r0 + a.c.rows_per_chunk < M ? r0 + a.c.rows_per_chunk : M;
    const Drop d = drop_here<DR>(a.c.drop);
    double s[N], q[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = q[j] = 0.0;
    if (col < C) {
        for (long long r = r0 + (threadIdx.x >> 3); r < r1; r += kRowsPerPass) {
            float gz[N], xh[N];
            gz_of_row<T, N>(a.c, d, reinterpret_cast<const T*>(a.g), a.ld_g, cc.mean + lc, cc.rstd + lc, cc.gamma + lc, cc.beta + lc, r, col,
                            gz, xh);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                s[j] += (double)gz[j];
                q[j] += (double)gz[j] * (double)xh[j];
            }
        }
    }
    write_partials<N>(s, q, lds, col, C, a.ws);
}

template <typename T, bool DR>
__global__ __launch_bounds__(kBlock) void bn_act_backward_kernel(BwdArgs a) {
    constexpr int N = VecOf<T>::N, SC = kLanesPerRow * N;
    __shared__ ColConst<SC> cc;
    __shared__ float c1s[SC], c2s[SC];
    const long long M = a.c.M, C = a.c.C, c0 = (long long)blockIdx.x * SC;
    if (threadIdx.x < SC) {
        const long long c = c0 + threadIdx.x;
        float mean = 0.0f, rstd = 0.0f, gm = 0.0f, bt = 0.0f, c1 = 0.0f, c2 = 0.0f;
        if (c < C) {
            mean = a.mean[c]; rstd = a.rstd[c]; gm = a.c.gamma[c]; bt = a.c.beta[c];
            double s = 0.0, q = 0.0;
            for (int k = 0; k < a.c.chunks; ++k) {
                s += a.ws[(long long)k * 2 * C + c];
                q += a.ws[(long long)k * 2 * C + C + c];
            }
            c1 = (float)(s / (double)M);
            c2 = (float)(q / (double)M);
            if (blockIdx.y == 0) {
                if (a.dbeta) a.dbeta[c] = (float)s;
                if (a.dgamma) a.dgamma[c] = (float)q;
            }
        }
        cc.mean[threadIdx.x] = mean; cc.rstd[threadIdx.x] = rstd; cc.gamma[threadIdx.x] = gm; cc.beta[threadIdx.x] = bt;
        c1s[threadIdx.x] = c1; c2s[threadIdx.x] = c2;
    }
    __syncthreads();
    const int lc = (threadIdx.x & 7) * N;
    const long long col = c0 + lc;
    const long long Cp = (C + 15) / 16 * 16;
    const long long r0 = (long long)blockIdx.y * a.c.rows_per_chunk;
    const long long r1 = r0 + a.c.rows_per_chunk < M ? r0 + a.c.rows_per_chunk : M;
    if (col >= Cp) return;
    const Drop d = drop_here<DR>(a.c.drop);
    for (long long r = r0 + (threadIdx.x >> 3); r < r1; r += kRowsPerPass) {
        float dz[N];
        if (col < C) {
            float gz[N], xh[N];
            gz_of_row<T, N>(a.c, d, reinterpret_cast<const T*>(a.g), a.ld_g, cc.mean + lc, cc.rstd + lc, cc.gamma + lc, cc.beta + lc, r, col,
                            gz, xh);
#pragma unroll
            for (int j = 0; j < N; ++j) dz[j] = (cc.gamma[lc + j] * cc.rstd[lc + j]) * ((gz[j] - c1s[lc + j]) - xh[j] * c2s[lc + j]);
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) dz[j] = 0.0f;
        }
        if (a.dzb) store_bf16(a.dzb + r * a.ld_dzb + col, col, C, dz);
        if (a.dzf && col < C) store_f32(a.dzf + r * a.ld_dzf + col, col, C, dz);
    }
}

// W' = gamma * rstd_run (.) rows of W, the part the two fold kernels share.  One rounding per result: the scale gamma * rstd_run stays
// in fp64 until the product is formed
__device__ __forceinline__ void fold_weight(const float* __restrict__ W, long long ldw, const float* __restrict__ gamma,
                                            const float* __restrict__ rvar, float eps, float* __restrict__ Wout, long long ld_out,
                                            long long N, long long K, long long tid, long long stride) {
    for (long long i = tid; i < N * K; i += stride) {
        const long long n = i / K, k = i - n * K;
        const double sc = (double)gamma[n] / sqrt((double)rvar[n] + (double)eps);
        Wout[n * ld_out + k] = (float)(sc * (double)W[n * ldw + k]);
    }
}

__global__ __launch_bounds__(kBlock) void bn_fold_kernel(const float* __restrict__ W, long long ldw, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ rmean,
                                                         const float* __restrict__ rvar, float eps, float* __restrict__ Wout,
                                                         long long ld_out, float* __restrict__ bias_out, float* __restrict__ rstd_out,
                                                         long long N, long long K) {
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    if (Wout) fold_weight(W, ldw, gamma, rvar, eps, Wout, ld_out, N, K, tid, stride);
    for (long long n = tid; n < N; n += stride) {
        const double rs = 1.0 / sqrt((double)rvar[n] + (double)eps);
        if (bias_out) bias_out[n] = (float)((double)beta[n] - (double)rmean[n] * ((double)gamma[n] * rs));
        if (rstd_out) rstd_out[n] = (float)rs;
    }
}

// the layer in front of the BatchNorm has a bias of its own: it is shifted by the running mean before the scale (the difference of two
// fp32 values is formed in fp64, where it is exact unless their exponents lie more than 29 binades apart)
__global__ __launch_bounds__(kBlock) void bn_fold_bias_kernel(const float* __restrict__ W, long long ldw,
                                                              const float* __restrict__ layer_bias, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ rmean,
                                                              const float* __restrict__ rvar, float eps, float* __restrict__ Wout,
                                                              long long ld_out, float* __restrict__ bias_out,
                                                              float* __restrict__ rstd_out, long long N, long long K) {
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    if (Wout) fold_weight(W, ldw, gamma, rvar, eps, Wout, ld_out, N, K, tid, stride);
    for (long long n = tid; n < N; n += stride) {
        const double rs = 1.0 / sqrt((double)rvar[n] + (double)eps);
        if (bias_out) bias_out[n] = (float)((double)beta[n] + ((double)layer_bias[n] - (double)rmean[n]) * ((double)gamma[n] * rs));
        if (rstd_out) rstd_out[n] = (float)rs;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
struct Launch {
    unsigned strips;
    int chunks;
    long long rows_per_chunk;
};

// column strips x row chunks: at least one workgroup per CU (256) where the batch has the rows for it, at most kMaxChunks chunks
Launch launch_of(int64_t M, int64_t C, int vec) {
    const int64_t sc = (int64_t)kLanesPerRow * vec, Cp = (C + 15) / 16 * 16;
    const int64_t strips = (Cp + sc - 1) / sc, passes = (M + kRowsPerPass - 1) / kRowsPerPass;
    int64_t want = (256 + strips - 1) / strips;
    if (want > kMaxChunks) want = kMaxChunks;
    if (want > passes) want = passes;
    if (want < 1) want = 1;
    Launch l;
    l.rows_per_chunk = (passes + want - 1) / want * kRowsPerPass;
    l.chunks = (int)((M + l.rows_per_chunk - 1) / l.rows_per_chunk);
    l.strips = (unsigned)strips;
    return l;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// a (M, >= C) matrix of `elem`-byte elements read or written with 16-byte vectors
inline bool rows_ok(const void* p, int64_t ld, int64_t width, int elem) {
    return p == nullptr || (aligned(p, 16) && ld >= width && (ld * elem) % 16 == 0);
}

// where a launch takes its stream position from: immediates (cell == nullptr, dr false) or the device cell of the _dr entries, in
// which case `offset` is the call's delta and `seed` is unused
struct Rng {
    bool dr;
    uint64_t seed, offset;
    const uint64_t* cell;
};

int drop_of(float p, const Rng& rng, Drop* d) {
    if (!(p >= 0.0f && p < 1.0f)) return DHAUG_EINVAL;                   // (a NaN fails the comparison)
    if (rng.dr && p > 0.0f && rng.cell == nullptr) return DHAUG_EINVAL;  // (p == 0: the cell is not read and may be NULL)
    if (rng.dr && p > 0.0f && (reinterpret_cast<uintptr_t>(rng.cell) & 7) != 0) return DHAUG_EALIGN;
    d->seed = rng.seed;
    d->offset = rng.offset;
    d->thresh = (unsigned)((double)p * 4294967296.0);
    d->inv_keep = 1.0f / (1.0f - p);
    d->cell = reinterpret_cast<const unsigned long long*>(rng.cell);
    return DHAUG_OK;
}

constexpr int64_t kMaxCols = 1ll << 30;

}  // namespace

extern "C" int dhaug_bn_partials(const void* z, int z_bf16, int64_t ld_z, int64_t M, int64_t C, void* workspace, void* stream) {
    DHAUG_CHECK(M >= 0 && C >= 0 && (z_bf16 == 0 || z_bf16 == 1), DHAUG_EINVAL);
    if (M == 0 || C == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(z); DHAUG_CHECK_PTR(workspace);
    DHAUG_CHECK(C < kMaxCols, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(rows_ok(z, ld_z, C, z_bf16 ? 2 : 4) && aligned(workspace, 8), DHAUG_EALIGN);
    const Launch l = launch_of(M, C, z_bf16 ? 8 : 4);
    const dim3 grid(l.strips, l.chunks);
    if (z_bf16)
        hipLaunchKernelGGL(bn_partials_kernel<uint16_t>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)z,
                           (long long)ld_z, (long long)M, (long long)C, l.rows_per_chunk, (double*)workspace);
    else
        hipLaunchKernelGGL(bn_partials_kernel<float>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const float*)z, (long long)ld_z,
                           (long long)M, (long long)C, l.rows_per_chunk, (double*)workspace);
    return dhaug_launch_status();
}

namespace {

template <typename T>
void launch_forward(bool dr, dim3 grid, hipStream_t stream, const FwdArgs& a) {
    if (dr)
        hipLaunchKernelGGL((bn_act_forward_kernel<T, true>), grid, dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((bn_act_forward_kernel<T, false>), grid, dim3(kBlock), 0, stream, a);
}

// dhaug_bn_act_forward and dhaug_bn_act_forward_dr: one set of checks, one argument block
int forward_launch(const void* z, int z_bf16, int64_t ld_z, const void* residual, int64_t ld_res, const float* gamma,
                   const float* beta, float* mean, float* rstd, const void* workspace, float* running_mean, float* running_var,
                   int64_t* num_batches_tracked, float momentum, float eps, float p, const Rng& rng, uint16_t* y_bf16, int64_t ld_yb,
                   float* y_f32, int64_t ld_yf, int64_t M, int64_t C, void* stream) {
    FwdArgs a;
    DHAUG_CHECK(M >= 0 && C >= 0 && (z_bf16 == 0 || z_bf16 == 1), DHAUG_EINVAL);
    const int drc = drop_of(p, rng, &a.c.drop);
    DHAUG_CHECK(drc == DHAUG_OK, drc);
    DHAUG_CHECK(eps >= 0.0f && momentum >= 0.0f && momentum <= 1.0f, DHAUG_EINVAL);
    if (M == 0 || C == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(z); DHAUG_CHECK_PTR(gamma); DHAUG_CHECK_PTR(beta); DHAUG_CHECK_PTR(mean); DHAUG_CHECK_PTR(rstd);
    DHAUG_CHECK(y_bf16 != nullptr || y_f32 != nullptr, DHAUG_EINVAL);
    // the running buffers come together, and only with batch statistics
    DHAUG_CHECK((running_mean == nullptr) == (running_var == nullptr), DHAUG_EINVAL);
    DHAUG_CHECK(workspace != nullptr || (running_mean == nullptr && num_batches_tracked == nullptr), DHAUG_EINVAL);
    DHAUG_CHECK(C < kMaxCols, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(workspace == nullptr || M >= 2, DHAUG_EUNSUPPORTED);       // batch statistics of one row (nn.BatchNorm1d raises)
    const int elem = z_bf16 ? 2 : 4;
    const int64_t Cp = (C + 15) / 16 * 16;
    DHAUG_CHECK(rows_ok(z, ld_z, C, elem) && rows_ok(residual, ld_res, C, elem) && rows_ok(y_bf16, ld_yb, Cp, 2) &&
                rows_ok(y_f32, ld_yf, C, 4), DHAUG_EALIGN);
    DHAUG_CHECK(aligned(gamma, 4) && aligned(beta, 4) && aligned(mean, 4) && aligned(rstd, 4) && aligned(running_mean, 4) &&
                aligned(running_var, 4) && aligned(workspace, 8) && aligned(num_batches_tracked, 8), DHAUG_EALIGN);
    const Launch l = launch_of(M, C, z_bf16 ? 8 : 4);
    a.c.z = z; a.c.ld_z = ld_z; a.c.gamma = gamma; a.c.beta = beta; a.c.M = M; a.c.C = C;
    a.c.rows_per_chunk = l.rows_per_chunk; a.c.chunks = l.chunks;
    a.res = residual; a.ld_res = ld_res; a.mean = mean; a.rstd = rstd; a.ws = (const double*)workspace;
    a.running_mean = running_mean; a.running_var = running_var; a.nbt = (long long*)num_batches_tracked;
    a.momentum = momentum; a.eps = eps; a.yb = y_bf16; a.ld_yb = ld_yb; a.yf = y_f32; a.ld_yf = ld_yf;
    const dim3 grid(l.strips, l.chunks);
    if (z_bf16)
        launch_forward<uint16_t>(rng.dr, grid, (hipStream_t)stream, a);
    else
        launch_forward<float>(rng.dr, grid, (hipStream_t)stream, a);
    return dhaug_launch_status();
}

}  // namespace

extern "C" int dhaug_bn_act_forward(const void* z, int z_bf16, int64_t ld_z, const void* residual, int64_t ld_res,
                                    const float* gamma, const float* beta, float* mean, float* rstd, const void* workspace,
                                    float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                                    float eps, float p, uint64_t seed, uint64_t offset, uint16_t* y_bf16, int64_t ld_yb,
                                    float* y_f32, int64_t ld_yf, int64_t M, int64_t C, void* stream) {
    return forward_launch(z, z_bf16, ld_z, residual, ld_res, gamma, beta, mean, rstd, workspace, running_mean, running_var,
                          num_batches_tracked, momentum, eps, p, Rng{false, seed, offset, nullptr}, y_bf16, ld_yb, y_f32, ld_yf, M, C,
                          stream);
}

extern "C" int dhaug_bn_act_forward_dr(const void* z, int z_bf16, int64_t ld_z, const void* residual, int64_t ld_res,
                                       const float* gamma, const float* beta, float* mean, float* rstd, const void* workspace,
                                       float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                                       float eps, float p, const uint64_t* rng_cell, uint64_t delta, uint16_t* y_bf16,
                                       int64_t ld_yb, float* y_f32, int64_t ld_yf, int64_t M, int64_t C, void* stream) {
    return forward_launch(z, z_bf16, ld_z, residual, ld_res, gamma, beta, mean, rstd, workspace, running_mean, running_var,
                          num_batches_tracked, momentum, eps, p, Rng{true, 0, delta, rng_cell}, y_bf16, ld_yb, y_f32, ld_yf, M, C,
                          stream);
}

namespace {

// argument checks and the argument block shared by the two backward launches
int backward_args(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma, const float* beta,
                  const float* mean, const float* rstd, float p, const Rng& rng, int64_t M, int64_t C, void* workspace, BwdArgs* a,
                  Launch* l, bool* empty) {
    *empty = false;
    DHAUG_CHECK(M >= 0 && C >= 0 && (z_bf16 == 0 || z_bf16 == 1), DHAUG_EINVAL);
    const int drc = drop_of(p, rng, &a->c.drop);
    DHAUG_CHECK(drc == DHAUG_OK, drc);
    if (M == 0 || C == 0) {
        *empty = true;
        return DHAUG_OK;
    }
    DHAUG_CHECK_PTR(z); DHAUG_CHECK_PTR(g); DHAUG_CHECK_PTR(gamma); DHAUG_CHECK_PTR(beta); DHAUG_CHECK_PTR(mean);
    DHAUG_CHECK_PTR(rstd); DHAUG_CHECK_PTR(workspace);
    DHAUG_CHECK(C < kMaxCols, DHAUG_EUNSUPPORTED);
    const int elem = z_bf16 ? 2 : 4;
    DHAUG_CHECK(rows_ok(z, ld_z, C, elem) && rows_ok(g, ld_g, C, elem), DHAUG_EALIGN);
    DHAUG_CHECK(aligned(gamma, 4) && aligned(beta, 4) && aligned(mean, 4) && aligned(rstd, 4) && aligned(workspace, 8), DHAUG_EALIGN);
    *l = launch_of(M, C, z_bf16 ? 8 : 4);
    a->c.z = z; a->c.ld_z = ld_z; a->c.gamma = gamma; a->c.beta = beta; a->c.M = M; a->c.C = C;
    a->c.rows_per_chunk = l->rows_per_chunk; a->c.chunks = l->chunks;
    a->g = g; a->ld_g = ld_g; a->mean = mean; a->rstd = rstd; a->ws = (double*)workspace;
    a->dzb = nullptr; a->ld_dzb = 0; a->dzf = nullptr; a->ld_dzf = 0; a->dgamma = nullptr; a->dbeta = nullptr;
    return DHAUG_OK;
}

template <typename T>
void launch_backward_partials(bool dr, dim3 grid, hipStream_t stream, const BwdArgs& a) {
    if (dr)
        hipLaunchKernelGGL((bn_act_backward_partials_kernel<T, true>), grid, dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((bn_act_backward_partials_kernel<T, false>), grid, dim3(kBlock), 0, stream, a);
}

template <typename T>
void launch_backward(bool dr, dim3 grid, hipStream_t stream, const BwdArgs& a) {
    if (dr)
        hipLaunchKernelGGL((bn_act_backward_kernel<T, true>), grid, dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((bn_act_backward_kernel<T, false>), grid, dim3(kBlock), 0, stream, a);
}

int backward_partials_launch(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma,
                             const float* beta, const float* mean, const float* rstd, float p, const Rng& rng, int64_t M, int64_t C,
                             void* workspace, void* stream) {
    BwdArgs a;
    Launch l;
    bool empty;
    const int rc = backward_args(z, z_bf16, ld_z, g, ld_g, gamma, beta, mean, rstd, p, rng, M, C, workspace, &a, &l, &empty);
    if (rc != DHAUG_OK || empty) return rc;
    const dim3 grid(l.strips, l.chunks);
    if (z_bf16)
        launch_backward_partials<uint16_t>(rng.dr, grid, (hipStream_t)stream, a);
    else
        launch_backward_partials<float>(rng.dr, grid, (hipStream_t)stream, a);
    return dhaug_launch_status();
}

int backward_launch(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma, const float* beta,
                    const float* mean, const float* rstd, float p, const Rng& rng, const void* workspace, uint16_t* dz_bf16,
                    int64_t ld_dzb, float* dz_f32, int64_t ld_dzf, float* dgamma, float* dbeta, int64_t M, int64_t C, void* stream) {
    BwdArgs a;
    Launch l;
    bool empty;
    const int rc = backward_args(z, z_bf16, ld_z, g, ld_g, gamma, beta, mean, rstd, p, rng, M, C, const_cast<void*>(workspace), &a,
                                 &l, &empty);
    if (rc != DHAUG_OK || empty) return rc;
    DHAUG_CHECK(dz_bf16 != nullptr || dz_f32 != nullptr, DHAUG_EINVAL);
    const int64_t Cp = (C + 15) / 16 * 16;
    DHAUG_CHECK(rows_ok(dz_bf16, ld_dzb, Cp, 2) && rows_ok(dz_f32, ld_dzf, C, 4) && aligned(dgamma, 4) && aligned(dbeta, 4),
                DHAUG_EALIGN);
    a.dzb = dz_bf16; a.ld_dzb = ld_dzb; a.dzf = dz_f32; a.ld_dzf = ld_dzf; a.dgamma = dgamma; a.dbeta = dbeta;
    const dim3 grid(l.strips, l.chunks);
    if (z_bf16)
        launch_backward<uint16_t>(rng.dr, grid, (hipStream_t)stream, a);
    else
        launch_backward<float>(rng.dr, grid, (hipStream_t)stream, a);
    return dhaug_launch_status();
}

}  // namespace

extern "C" int dhaug_bn_act_backward_partials(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g,
                                              const float* gamma, const float* beta, const float* mean, const float* rstd, float p,
                                              uint64_t seed, uint64_t offset, int64_t M, int64_t C, void* workspace, void* stream) {
    return backward_partials_launch(z, z_bf16, ld_z, g, ld_g, gamma, beta, mean, rstd, p, Rng{false, seed, offset, nullptr}, M, C,
                                    workspace, stream);
}

extern "C" int dhaug_bn_act_backward_partials_dr(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g,
                                                 const float* gamma, const float* beta, const float* mean, const float* rstd,
                                                 float p, const uint64_t* rng_cell, uint64_t delta, int64_t M, int64_t C,
                                                 void* workspace, void* stream) {
    return backward_partials_launch(z, z_bf16, ld_z, g, ld_g, gamma, beta, mean, rstd, p, Rng{true, 0, delta, rng_cell}, M, C,
                                    workspace, stream);
}

extern "C" int dhaug_bn_act_backward(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma,
                                     const float* beta, const float* mean, const float* rstd, float p, uint64_t seed,
                                     uint64_t offset, const void* workspace, uint16_t* dz_bf16, int64_t ld_dzb, float* dz_f32,
                                     int64_t ld_dzf, float* dgamma, float* dbeta, int64_t M, int64_t C, void* stream) {
    return backward_launch(z, z_bf16, ld_z, g, ld_g, gamma, beta, mean, rstd, p, Rng{false, seed, offset, nullptr}, workspace, dz_bf16,
                           ld_dzb, dz_f32, ld_dzf, dgamma, dbeta, M, C, stream);
}

extern "C" int dhaug_bn_act_backward_dr(const void* z, int z_bf16, int64_t ld_z, const void* g, int64_t ld_g, const float* gamma,
                                        const float* beta, const float* mean, const float* rstd, float p, const uint64_t* rng_cell,
                                        uint64_t delta, const void* workspace, uint16_t* dz_bf16, int64_t ld_dzb, float* dz_f32,
                                        int64_t ld_dzf, float* dgamma, float* dbeta, int64_t M, int64_t C, void* stream) {
    return backward_launch(z, z_bf16, ld_z, g, ld_g, gamma, beta, mean, rstd, p, Rng{true, 0, delta, rng_cell}, workspace, dz_bf16,
                           ld_dzb, dz_f32, ld_dzf, dgamma, dbeta, M, C, stream);
}

namespace {

// the two fold entry points: layer_bias == nullptr launches dhaug_bn_fold's own kernel
int fold_launch(const float* W, int64_t ldw, const float* layer_bias, const float* gamma, const float* beta,
                const float* running_mean, const float* running_var, float eps, float* W_out, int64_t ld_out, float* bias_out,
                float* rstd_out, int64_t N, int64_t K, void* stream) {
    DHAUG_CHECK(N >= 0 && K >= 0 && eps >= 0.0f, DHAUG_EINVAL);
    if (N == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(gamma); DHAUG_CHECK_PTR(beta); DHAUG_CHECK_PTR(running_mean); DHAUG_CHECK_PTR(running_var);
    DHAUG_CHECK(W_out != nullptr || bias_out != nullptr || rstd_out != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(W_out == nullptr || K == 0 || W != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(N < kMaxCols && K < kMaxCols, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(W_out == nullptr || (ldw >= K && ld_out >= K), DHAUG_EALIGN);
    DHAUG_CHECK(aligned(W, 4) && aligned(W_out, 4) && aligned(gamma, 4) && aligned(beta, 4) && aligned(running_mean, 4) &&
                aligned(running_var, 4) && aligned(bias_out, 4) && aligned(rstd_out, 4) && aligned(layer_bias, 4), DHAUG_EALIGN);
    const int64_t items = W_out ? (N * K > N ? N * K : N) : N;
    const dim3 grid(dhaug_stream_grid(items, kBlock));
    if (layer_bias)
        hipLaunchKernelGGL(bn_fold_bias_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, W, (long long)ldw, layer_bias, gamma, beta,
                           running_mean, running_var, eps, K == 0 ? nullptr : W_out, (long long)ld_out, bias_out, rstd_out,
                           (long long)N, (long long)K);
    else
        hipLaunchKernelGGL(bn_fold_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, W, (long long)ldw, gamma, beta, running_mean,
                           running_var, eps, K == 0 ? nullptr : W_out, (long long)ld_out, bias_out, rstd_out, (long long)N,
                           (long long)K);
    return dhaug_launch_status();
}

}  // namespace

extern "C" int dhaug_bn_fold(const float* W, int64_t ldw, const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, float* W_out, int64_t ld_out, float* bias_out, float* rstd_out,
                             int64_t N, int64_t K, void* stream) {
    return fold_launch(W, ldw, nullptr, gamma, beta, running_mean, running_var, eps, W_out, ld_out, bias_out, rstd_out, N, K, stream);
}

extern "C" int dhaug_bn_fold_bias(const float* W, int64_t ldw, const float* layer_bias, const float* gamma, const float* beta,
                                  const float* running_mean, const float* running_var, float eps, float* W_out, int64_t ld_out,
                                  float* bias_out, float* rstd_out, int64_t N, int64_t K, void* stream) {
    return fold_launch(W, ldw, layer_bias, gamma, beta, running_mean, running_var, eps, W_out, ld_out, bias_out, rstd_out, N, K,
                       stream);
}
