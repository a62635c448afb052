// Copy-out of a fused kernel's fp32 output tile whose rows are contiguous in global memory (ld == N): used by the bf16 kernel
// (dhaug_mlp.hip, 256 threads).  The f16x3 kernel (dhaug_mlp_x3.hip, 512 threads, the same staging image) keeps its rolled loop:
// with this copy its register allocation spilled more (scratch 224 -> 312 bytes per lane) and --precision parity was 6 % slower.
//
// The staging image in LDS is [128 rows][OUTC_PITCH floats], columns [0, N) of a row live, N <= 64.  In memory the tile's live
// part is ONE linear array of rows_live * N floats at out + m0 * N -- 16-byte aligned for every N (m0 is a multiple of 128, the
// base is checked by the planner) -- so it leaves as 16-byte groups: thread i takes groups i, i + THREADS, ...  A thread first
// issues ALL its LDS reads, then its stores: one LDS round trip per tile instead of one per dword (the rolled loop it
// replaces: 17.5 trips of ~30 instructions for the generator's 35-wide head, each waiting for its ds_read).
#pragma once
#include <stdint.h>

constexpr int OUTC_PITCH = 68;                                       // floats per staging row (both kernels' OUT_PITCH)
constexpr int OUTC_BM = 128;                                         // rows per tile
constexpr int OUTC_SHIFT = 19;

// row of linear element e (e < 128 * 64, 1 <= N <= 64): floor(e / N) == (e * magic(N)) >> 19 in 32-bit unsigned arithmetic.
// With magic = floor(2^19 / N) + 1 and d = magic * N - 2^19 (1 <= d <= N) the quotient is exact while e * d < 2^19: 8191 * 64
// = 524 224 < 524 288; the product stays below 2^32 (N = 1: 8191 * 524 289 = 4 294 451 199) and both factors below 2^24.
// tests/test_mlp_out_cpu.py walks every (e, N) with the same integer arithmetic.
__host__ __device__ inline uint32_t outc_magic(int N) { return (1u << OUTC_SHIFT) / (uint32_t)N + 1u; }

typedef float outc_f32x4 __attribute__((ext_vector_type(4)));

// st: the staging image; out: the tensor's base (16-byte aligned, row length N); magic: outc_magic(N), from the host; rows
// [m0, min(m0 + 128, M)) are written, nothing else; no staging element beyond a live row's columns [0, N) is read (the element index is clamped to the last live one).
template <int THREADS>
__device__ __forceinline__ void outc_copy_linear(const float* st, float* out, int N, uint32_t magic, long long m0, long long M, int tid) {
    constexpr int NG = OUTC_BM * 64 / 4 / THREADS;                           // groups per thread at N = 64
    const long long left = M - m0;
    const int total = (left < OUTC_BM ? (int)left : OUTC_BM) * N, last = total - 1;
    const uint32_t skip = 4u * (uint32_t)(OUTC_PITCH - N);
    const unsigned char* img = reinterpret_cast<const unsigned char*>(st);
    float* p = out + m0 * N;
    float v[NG][4];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        if (4 * THREADS * j >= total) break;                                 // (workgroup-uniform)
        const int e0 = 4 * (tid + THREADS * j);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t e = (uint32_t)(e0 + q < last ? e0 + q : last);
            const uint32_t row = (uint32_t)__umul24(e, magic) >> OUTC_SHIFT;
            v[j][q] = *reinterpret_cast<const float*>(img + (4u * e + (uint32_t)__umul24(row, skip)));   // (row * PITCH + e - row * N) floats
        }
    }
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        if (4 * THREADS * j >= total) break;
        const int e0 = 4 * (tid + THREADS * j);
        if (e0 + 3 < total) {
            *reinterpret_cast<outc_f32x4*>(p + e0) = outc_f32x4{v[j][0], v[j][1], v[j][2], v[j][3]};
        } else {                                                             // the ragged last tile's total % 4 floats
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (e0 + q < total) p[e0 + q] = v[j][q];
        }
    }
}
