// Per-value arithmetic of the DOF angle histograms (dhaug_dof.hip): the reference's one-degree table
//     each_DOF_distribution[dof][int(angle) + 180] += 1          (R/models_Fk_GAN/special_operate.py:359-364)
// as one function that host and device compile from the same source (tests/dofcheck builds it for the host under ASan + UBSan).
//
// int(angle) truncates towards zero: -0.5 and 0.999 both land in bin 180, which is therefore two degrees wide; every other bin
// b holds [b - 180, b - 179) on the positive side and (b - 181, b - 180] on the negative one.  The table has 361 bins, so
// 180.5 (bin 360) and -180.9 (bin 0) are still inside.  Past that the reference wraps (a negative index) or raises; here the
// value is counted in the end bin AND flagged, and a NaN enters no bin.
//
// The range check is made on the truncated FLOAT: no float-to-int conversion happens before the value is known to lie in
// [-180, 180] (converting NaN, inf or 1e30 to int is undefined behaviour -- UBSan's float-cast-overflow check in tests/dofcheck
// is the guard).  NaN and inf are recognised by their bit patterns, so the classification does not hang on -ffinite-math-only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "dhaug.h"

namespace dhaug_dof {

constexpr int kBins = DHAUG_DOF_BINS;
constexpr int F_NAN = 1;          // no bin (the function returns -1), no moment
constexpr int F_OUTSIDE = 2;      // |trunc(a)| > 180 or +-inf: counted in the end bin and in `outside`
constexpr int F_INF = 4;          // +-inf: stays out of sum / sumsq (set together with F_OUTSIDE)

// bin of one angle (0..360, or -1 for a NaN) and its flags
__host__ __device__ __forceinline__ int bin_of(float a, int& flags) {
    const uint32_t mag = __builtin_bit_cast(uint32_t, a) & 0x7fffffffu;
    if (mag > 0x7f800000u) {
        flags = F_NAN;
        return -1;
    }
    const bool neg = (__builtin_bit_cast(uint32_t, a) >> 31) != 0;
    if (mag == 0x7f800000u) {
        flags = F_OUTSIDE | F_INF;
        return neg ? 0 : kBins - 1;
    }
    const float t = truncf(a);
    if (t > 180.0f) {
        flags = F_OUTSIDE;
        return kBins - 1;
    }
    if (t < -180.0f) {
        flags = F_OUTSIDE;
        return 0;
    }
    flags = 0;
    return (int)t + 180;          // t is an integer in [-180, 180]: the conversion is exact
}

// Order of the fp32 values as signed integers (-0 below +0; not for NaN): min and max are taken on these keys, so the
// result does not depend on the order in which values meet and the zero that comes out is a defined one (min: -0 if any,
// max: +0 if any).
__host__ __device__ __forceinline__ int32_t order_key(float a) {
    const int32_t b = __builtin_bit_cast(int32_t, a);
    return b < 0 ? (int32_t)(b ^ 0x7fffffff) : b;
}
__host__ __device__ __forceinline__ float key_value(int32_t k) {
    return __builtin_bit_cast(float, k < 0 ? (int32_t)(k ^ 0x7fffffff) : k);
}

}  // namespace dhaug_dof
