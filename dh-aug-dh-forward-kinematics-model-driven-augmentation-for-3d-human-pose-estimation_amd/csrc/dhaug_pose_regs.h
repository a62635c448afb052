// One 16-joint pose-frame per lane, held in registers: what dhaug_pair_batch (dhaug_posetrain.hip) and dhaug_clip_pair_batch
// (dhaug_clip.hip) share.  12 (3D) or 8 (2D) float4 loads / stores per pose; the H36M left/right flip is resolved at compile time,
// so every index into the register arrays is a constant (an array indexed by a run-time value would go to scratch).
#pragma once
#include <hip/hip_runtime.h>

namespace dhaug_pose_regs {

// joint j of the flipped pose is joint flip_src(j) of the pose (swap [4,5,6,10,11,12] <-> [1,2,3,13,14,15])
__device__ __forceinline__ constexpr int flip_src(int j) {
    return j == 1 ? 4 : j == 2 ? 5 : j == 3 ? 6 : j == 4 ? 1 : j == 5 ? 2 : j == 6 ? 3 : j == 10 ? 13 : j == 11 ? 14 : j == 12 ? 15
         : j == 13 ? 10 : j == 14 ? 11 : j == 15 ? 12 : j;
}

template <int C>
__device__ __forceinline__ void load_pose(const float* src, float (&x)[16 * C]) {
#pragma unroll
    for (int q = 0; q < 4 * C; ++q) {
        const float4 v = reinterpret_cast<const float4*>(src)[q];
        x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
    }
}
template <int C>
__device__ __forceinline__ void store_pose(float* dst, const float (&x)[16 * C]) {
#pragma unroll
    for (int q = 0; q < 4 * C; ++q)
        reinterpret_cast<float4*>(dst)[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}
template <int C>
__device__ __forceinline__ void flip_pose(const float (&x)[16 * C], float (&y)[16 * C]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        y[C * j] = -x[C * flip_src(j)];
#pragma unroll
        for (int c = 1; c < C; ++c) y[C * j + c] = x[C * flip_src(j) + c];
    }
}

}  // namespace dhaug_pose_regs
