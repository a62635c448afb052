// The VideoPose3D family of R/utils/loss.py as training criteria: n_mpjpe :167-177, weighted_mpjpe :26-32 and mpjpe_byjoint
// :17-23, forward AND backward, with the conventions of dhaug_pose_mpjpe (dhaug_posetrain.hip) and the layout of
// dhaug_pose_scaled_errors (dhaug_eval_detail.hip).
//
//  dhaug_pose_nmpjpe    launch 1, per pose of (16, 3) in fp64 from the fp32 values: pp = sum p.p, tp = sum t.p, s = tp / pp (the
//                       reference's two means over the joints cancel), r_j = s p_j - t_j, e_j = |r_j|, u_j = r_j / e_j (exactly 0
//                       where e_j == 0), a = sum_j u_j.p_j, and with J = 16 P joints
//                           grad_k = fl32((s u_k + a (t_k - 2 s p_k) / pp) / J)       -- rounded once;
//                       that is torch's autograd of the reference's expression: d e_j / d p = s u_j + (u_j.p_j) ds/dp with
//                       ds/dp = (t - 2 s p) / pp.  e summed in fp64 per workgroup -> one partial each.  Launch 2 (one wave): the
//                       partials in index order -> loss = fl32(sum / J) and the meter record.
//  dhaug_pose_wmpjpe    mean(w |p - t|) the same way: grad = fl32(w d / (e J)), exactly 0 where e == 0, w e summed.  w: one value
//                       per pose, per pose and joint, or per joint shared by all poses.
//  dhaug_pose_byjoint_backward   the backward of mean over the rows of |p - t| per column: grad[r, c] = fl32(cot[c] d / (e rows)),
//                       exactly 0 where e == 0.  One launch, four joints per lane.
//
// Layout of the first two: a lane owns a quad of 4 joints (12 floats = 3 float4 per operand) in registers, 4 lanes a pose, a
// workgroup of 256 lanes 64 poses per trip of a grid-stride loop: a wave reads 16 whole poses as one contiguous stretch.  A pose's
// sums (tp, pp, then a) meet in two-level xor butterflies over its 4 lanes, so all four hold the same bits, every input element is
// read once and every gradient element written once.  The loop runs the same number of times in every lane of the workgroup: the
// butterflies never meet an idle lane (lanes past P carry zeros and neither store nor add).  A NaN or an all-zero predicted pose
// (0 / 0) stays inside its pose's 4 lanes = 48 gradient values, and reaches the loss.
// Bases on a 16-byte boundary take the float4 path, others scalar loads and stores of the same values.
// No atomics anywhere: the same call sequence gives the same bits.
#include "dhaug_common.h"

#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kPoseBlock = 64;                  // poses per workgroup and trip (4 lanes each)
constexpr int kMaxGrid = 2048;                  // partials: DHAUG_POSETRAIN_WORKSPACE_BYTES / 8

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// valid in lane 0: a butterfly per wave, then the 4 waves in order
__device__ __forceinline__ double block_sum(double v, double* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// 12 consecutive floats (4 joints) at p
template <bool VEC>
__device__ __forceinline__ void load12(const float* p, float f[12]) {
    if (VEC) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1],
                     c = reinterpret_cast<const float4*>(p)[2];
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
        f[8] = c.x; f[9] = c.y; f[10] = c.z; f[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) f[k] = p[k];
    }
}
template <bool VEC>
__device__ __forceinline__ void store12(float* p, const float f[12]) {
    if (VEC) {
        reinterpret_cast<float4*>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
        reinterpret_cast<float4*>(p)[2] = make_float4(f[8], f[9], f[10], f[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) p[k] = f[k];
    }
}

struct CritArgs {
    const float* pred;
    const float* tgt;
    const float* w;          // MODE 1: (P,)  2: (P, 16)  3: (16,)
    float* grad;
    double* partials;        // (gridDim.x,)
    long long P;
};

// MODE 0: N-MPJPE.  MODE 1 / 2 / 3: weighted MPJPE with DHAUG_WMPJPE_PER_POSE / _PER_JOINT / _SHARED weights.
template <int MODE, bool VEC>
__global__ __launch_bounds__(kBlock) void pose_criterion_kernel(CritArgs a) {
    __shared__ double lds[4];
    const int t = threadIdx.x, q = t & 3;
    const double nj = 16.0 * (double)a.P;
    double acc = 0.0;
    float ws[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (MODE == 3) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[j] = a.w[4 * q + j];
    }
    for (long long base = (long long)blockIdx.x * kPoseBlock; base < a.P; base += (long long)gridDim.x * kPoseBlock) {
        const long long n = base + (t >> 2);
        const bool valid = n < a.P;
        float y[12], x[12], g[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) y[k] = x[k] = 0.0f;
        float wj[4] = {ws[0], ws[1], ws[2], ws[3]};
        if (valid) {
            load12<VEC>(a.pred + n * 48 + 12 * q, y);
            load12<VEC>(a.tgt + n * 48 + 12 * q, x);
            if (MODE == 1) {
                wj[0] = wj[1] = wj[2] = wj[3] = a.w[n];
            } else if (MODE == 2) {
                const float4 w4 = reinterpret_cast<const float4*>(a.w + n * 16)[q];
                wj[0] = w4.x; wj[1] = w4.y; wj[2] = w4.z; wj[3] = w4.w;
            }
        }
        double e_sum = 0.0;
        if (MODE == 0) {
            // the scale: the tree of scaled_errors_kernel (a joint's 3 products, the lane's 4 joints in pairs, the pose's 4 lanes)
            double tj[4], pj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double y0 = y[3 * j], y1 = y[3 * j + 1], y2 = y[3 * j + 2];
                tj[j] = (double)x[3 * j] * y0 + (double)x[3 * j + 1] * y1 + (double)x[3 * j + 2] * y2;
                pj[j] = y0 * y0 + y1 * y1 + y2 * y2;
            }
            double tp = (tj[0] + tj[1]) + (tj[2] + tj[3]), pp = (pj[0] + pj[1]) + (pj[2] + pj[3]);
            tp += __shfl_xor(tp, 1, 64); pp += __shfl_xor(pp, 1, 64);
            tp += __shfl_xor(tp, 2, 64); pp += __shfl_xor(pp, 2, 64);
            const double s = tp / pp;                              // 0 / 0 = NaN, as the reference
            double u[12], uj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double r0 = s * (double)y[3 * j] - (double)x[3 * j], r1 = s * (double)y[3 * j + 1] - (double)x[3 * j + 1],
                             r2 = s * (double)y[3 * j + 2] - (double)x[3 * j + 2];
                const double e = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
                const bool zero = e == 0.0;
                u[3 * j] = zero ? 0.0 : r0 / e;
                u[3 * j + 1] = zero ? 0.0 : r1 / e;
                u[3 * j + 2] = zero ? 0.0 : r2 / e;
                uj[j] = u[3 * j] * (double)y[3 * j] + u[3 * j + 1] * (double)y[3 * j + 1] + u[3 * j + 2] * (double)y[3 * j + 2];
                e_sum += e;
            }
            double av = (uj[0] + uj[1]) + (uj[2] + uj[3]);
            av += __shfl_xor(av, 1, 64);
            av += __shfl_xor(av, 2, 64);
            const double c = av / pp, s2 = 2.0 * s;
#pragma unroll
            for (int k = 0; k < 12; ++k) g[k] = (float)((s * u[k] + c * ((double)x[k] - s2 * (double)y[k])) / nj);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d0 = (double)y[3 * j] - (double)x[3 * j], d1 = (double)y[3 * j + 1] - (double)x[3 * j + 1],
                             d2 = (double)y[3 * j + 2] - (double)x[3 * j + 2];
                const double e = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
                const double w = (double)wj[j], den = e * nj;
                const bool zero = e == 0.0;
                g[3 * j] = zero ? 0.0f : (float)(w * d0 / den);
                g[3 * j + 1] = zero ? 0.0f : (float)(w * d1 / den);
                g[3 * j + 2] = zero ? 0.0f : (float)(w * d2 / den);
                e_sum += w * e;
            }
        }
        if (valid) {
            store12<VEC>(a.grad + n * 48 + 12 * q, g);
            acc += e_sum;
        }
    }
    acc = block_sum(acc, lds);
    if (t == 0) a.partials[blockIdx.x] = acc;
}

// one wave: loss = fl32(sum / joints); the meter takes what AverageMeter.update(loss.item(), poses) adds.  (pose_mse_finish_kernel
// of dhaug_posetrain.hip, restated: that one is private to its translation unit.)
__global__ __launch_bounds__(64) void criterion_finish_kernel(const double* __restrict__ partials, int nparts, double joints,
                                                              long long poses, float* __restrict__ loss,
                                                              dhaug_loss_meter* __restrict__ meter) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 64) s += partials[b];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const float l = (float)(s / joints);
        *loss = l;
        if (meter) {
            meter->sum_loss_x_poses += (double)l * (double)poses;
            meter->poses += poses;
            meter->steps += 1;
        }
    }
}

// one joint of the per-joint backward: cot d / (e rows) rounded to fp32 once -- 0 where the distance is 0, NaN where it is NaN
__device__ __forceinline__ void byjoint_joint(double dx, double dy, double dz, double cot, double rows, float& gx, float& gy,
                                              float& gz) {
    const double e = sqrt(dx * dx + dy * dy + dz * dz);
    const double den = e * rows;
    const bool zero = e == 0.0;
    gx = zero ? 0.0f : (float)(cot * dx / den);
    gy = zero ? 0.0f : (float)(cot * dy / den);
    gz = zero ? 0.0f : (float)(cot * dz / den);
}

__global__ __launch_bounds__(kBlock) void byjoint_backward_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                  const float* __restrict__ cot, float* __restrict__ grad,
                                                                  long long joints, long long cols, double rows, int vec) {
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    const long long n4 = vec ? joints >> 2 : 0;                  // groups of four joints = 12 floats = three float4
    for (long long i = tid; i < n4; i += stride) {
        float y[12], x[12], g[12];
        load12<true>(pred + 12 * i, y);
        load12<true>(tgt + 12 * i, x);
        long long c = (4 * i) % cols;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            byjoint_joint((double)y[3 * j] - (double)x[3 * j], (double)y[3 * j + 1] - (double)x[3 * j + 1],
                          (double)y[3 * j + 2] - (double)x[3 * j + 2], (double)cot[c], rows, g[3 * j], g[3 * j + 1], g[3 * j + 2]);
            c = c + 1 == cols ? 0 : c + 1;
        }
        store12<true>(grad + 12 * i, g);
    }
    for (long long j = 4 * n4 + tid; j < joints; j += stride) {
        const float* p = pred + 3 * j;
        const float* t = tgt + 3 * j;
        float gx, gy, gz;
        byjoint_joint((double)p[0] - (double)t[0], (double)p[1] - (double)t[1], (double)p[2] - (double)t[2], (double)cot[j % cols],
                      rows, gx, gy, gz);
        grad[3 * j] = gx; grad[3 * j + 1] = gy; grad[3 * j + 2] = gz;
    }
}

// dhaug_pose_nmpjpe (mode 0, w unused) and dhaug_pose_wmpjpe (mode 1..3): one set of checks, one launch shape
int criterion_launch(const float* pred, const float* tgt, int64_t P, const float* w, int mode, int64_t poses, float* grad,
                     float* loss, void* meter, void* workspace, void* stream) {
    DHAUG_CHECK(P >= 0 && poses >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(grad != nullptr && loss != nullptr && workspace != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(P < (1ll << 31), DHAUG_EUNSUPPORTED);
    if (P == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pred); DHAUG_CHECK_PTR(tgt);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt) | reinterpret_cast<uintptr_t>(grad) |
                 reinterpret_cast<uintptr_t>(loss)) % 4 == 0, DHAUG_EALIGN);
    DHAUG_CHECK(reinterpret_cast<uintptr_t>(w) % (mode == DHAUG_WMPJPE_PER_JOINT ? 16 : 4) == 0, DHAUG_EALIGN);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(meter)) % 8 == 0, DHAUG_EALIGN);
    const bool vec = dhaug_aligned16(pred) && dhaug_aligned16(tgt) && dhaug_aligned16(grad);
    const int grid = dhaug_stream_grid(P, kPoseBlock, kMaxGrid);
    const hipStream_t s = (hipStream_t)stream;
    CritArgs a;
    a.pred = pred; a.tgt = tgt; a.w = w; a.grad = grad;
    a.partials = reinterpret_cast<double*>(workspace);
    a.P = P;
#define DHAUG_CRIT_LAUNCH(M)                                                                                        \
    if (vec) hipLaunchKernelGGL((pose_criterion_kernel<M, true>), dim3(grid), dim3(kBlock), 0, s, a);               \
    else hipLaunchKernelGGL((pose_criterion_kernel<M, false>), dim3(grid), dim3(kBlock), 0, s, a)
    switch (mode) {
        case 0: DHAUG_CRIT_LAUNCH(0); break;
        case DHAUG_WMPJPE_PER_POSE: DHAUG_CRIT_LAUNCH(1); break;
        case DHAUG_WMPJPE_PER_JOINT: DHAUG_CRIT_LAUNCH(2); break;
        default: DHAUG_CRIT_LAUNCH(3); break;
    }
#undef DHAUG_CRIT_LAUNCH
    hipLaunchKernelGGL(criterion_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)a.partials, grid, 16.0 * (double)P,
                       (long long)poses, loss, reinterpret_cast<dhaug_loss_meter*>(meter));
    return dhaug_launch_status();
}

}  // namespace

extern "C" int dhaug_pose_nmpjpe(const float* pred, const float* tgt, int64_t P, int64_t poses, float* grad, float* loss,
                                 void* meter, void* workspace, void* stream) {
    return criterion_launch(pred, tgt, P, nullptr, 0, poses, grad, loss, meter, workspace, stream);
}

extern "C" int dhaug_pose_wmpjpe(const float* pred, const float* tgt, int64_t P, const float* w, int w_mode, int64_t poses,
                                 float* grad, float* loss, void* meter, void* workspace, void* stream) {
    DHAUG_CHECK(w != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(w_mode == DHAUG_WMPJPE_PER_POSE || w_mode == DHAUG_WMPJPE_PER_JOINT || w_mode == DHAUG_WMPJPE_SHARED, DHAUG_EINVAL);
    return criterion_launch(pred, tgt, P, w, w_mode, poses, grad, loss, meter, workspace, stream);
}

extern "C" int dhaug_pose_byjoint_backward(const float* pred, const float* tgt, int64_t rows, int64_t cols, const float* cot,
                                           float* grad, void* stream) {
    DHAUG_CHECK(rows >= 0 && cols >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(rows < (1ll << 31) && cols < (1ll << 31), DHAUG_EUNSUPPORTED);
    if (rows == 0 || cols == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pred); DHAUG_CHECK_PTR(tgt); DHAUG_CHECK_PTR(cot); DHAUG_CHECK_PTR(grad);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt) | reinterpret_cast<uintptr_t>(grad) |
                 reinterpret_cast<uintptr_t>(cot)) % 4 == 0, DHAUG_EALIGN);
    const int vec = dhaug_aligned16(pred) && dhaug_aligned16(tgt) && dhaug_aligned16(grad);
    const int64_t joints = rows * cols;
    hipLaunchKernelGGL(byjoint_backward_kernel, dim3(dhaug_stream_grid((joints + 3) / 4, kBlock, kMaxGrid)), dim3(kBlock), 0,
                       (hipStream_t)stream, pred, tgt, cot, grad, (long long)joints, (long long)cols, (double)rows, vec);
    return dhaug_launch_status();
}
