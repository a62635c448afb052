// What surrounds the posenet call in the training loops (R/function_aug/model_pos_train.py:13-83 and
// R/models_Fk_GAN/video_mode_operate.py:532-765): the batch one iteration consumes, nn.MSELoss forward + backward with the
// epoch's loss meter, and clip_grad_norm_ + Adam.step() on the optimizer's flat buffers.  The posenet itself stays a torch module.
//
//  dhaug_pair_batch     one launch: gather (optional int64 row indices), root-centre the 3D rows per frame, and the flipped /
//                       frame-reversed copies the up-to-four steps of an iteration read.  One pose-frame per lane: 12 (3D) or
//                       8 (2D) float4 loads, the permutation resolved at compile time in registers, float4 stores.  Data
//                       movement, one fp32 subtraction and a sign flip: equal to the torch expressions bit for bit.
//  dhaug_pose_mse       launch 1: grad = (pred - tgt) * fl32(2 / numel), squares summed in fp64 per workgroup (butterfly over
//                       the wave, the four waves in order) -> one partial each; launch 2 (one wave): the partials in index order
//                       -> loss (rounded to fp32 once) and the meter record.
//  dhaug_pose_mpjpe     mean(norm(pred - tgt, dim=-1)) (R/utils/loss.py:8-14) forward + backward with the same two launches.
//                       Launch 1, per joint: d = pred - tgt in fp64 (exact), e = sqrt(dx^2 + dy^2 + dz^2) in fp64,
//                       grad = fl32(d / (e * joints)) -- rounded once -- and exactly 0 where e == 0 (the zero subgradient torch's
//                       autograd gives there); e summed in fp64 per workgroup as above.  Four joints per lane = three float4 loads
//                       per tensor; a scalar path for the joints % 4 tail and for bases off a 16-byte boundary.  Launch 2 is
//                       dhaug_pose_mse's: loss = fl32(sum / joints) and the meter record.
//                       A NaN input gives a NaN loss and a NaN gradient for that joint only.  Not reproduced: the fp32 overflow
//                       of the reference's squares (|d| >~ 1.8e19 gives an inf loss there; here the distance is formed in fp64),
//                       and its zero gradient for a distance too small for fp32 squares (here: the true unit vector / joints).
//  dhaug_grad_sumsq     per-workgroup fp64 partials of (g * grad_scale)^2 over a partition fixed by n (and the pointer's
//                       alignment); one thread also advances the optimizer's step count (the Adam launch behind it reads it:
//                       stream order is the synchronisation).
//  dhaug_adam_clip_step adam_dev_kernel's arithmetic (dhaug_elem.hip) with the clip coefficient.  Prologue: every workgroup adds the
//                       partials in the same order (the launch-boundary reduce: no third launch), so all of them hold the same
//                       norm and coef.  coef == 1 runs adam_dev_kernel's loop as it is written there: its bits.
//  dhaug_adam_clip_step_lr  the same kernel instantiated with the learning rate read from one device float (a captured launch follows
//                       the schedule); for an equal lr the same bits.
//  dhaug_u64_add        *cell += value on a device uint64: the base of the posenet's device dropout stream, advanced once per step.
// No atomics anywhere: the same call sequence gives the same bits.
#include "dhaug_common.h"
#include "dhaug_pose_regs.h"

#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kPairBlock = 64;                                  // one pose-frame per lane: small workgroups spread a 1 024-pose batch
constexpr int kMaxGrid = 2048;                                  // partials of dhaug_pose_mse / dhaug_pose_mpjpe
constexpr int kSumsqMaxGrid = DHAUG_GRAD_SUMSQ_MAX_PARTIALS;    // partials of dhaug_grad_sumsq: every Adam workgroup re-adds them

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the same value in every thread: butterfly per wave, then the four waves in order
__device__ __forceinline__ double block_sum(double v, double* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------------------------ pair batch
struct PairArgs {
    const float* p3;
    const float* p2;
    const long long* idx;
    float* tgt;
    float* tgt_flip;
    float* inp;
    float* inp_flip;
    float* inp_back;
    float* inp_flip_back;
    long long n;
    int F3, F2;
};

// one pose-frame per lane in registers: dhaug_pose_regs.h (shared with dhaug_clip_pair_batch)
using namespace dhaug_pose_regs;

__global__ __launch_bounds__(kPairBlock) void pair_batch_kernel(PairArgs a) {
    const long long n3 = a.p3 ? a.n * a.F3 : 0, total = n3 + (a.p2 ? a.n * a.F2 : 0);
    for (long long item = (long long)blockIdx.x * kPairBlock + threadIdx.x; item < total; item += (long long)gridDim.x * kPairBlock) {
        if (item < n3) {
            const long long i = item / a.F3;
            const int f = (int)(item - i * a.F3);
            const long long row = a.idx ? a.idx[i] : i;
            float x[48], y[48];
            load_pose<3>(a.p3 + (row * a.F3 + f) * 48, x);
            const float r0 = x[0], r1 = x[1], r2 = x[2];
#pragma unroll
            for (int j = 0; j < 16; ++j) { x[3 * j] -= r0; x[3 * j + 1] -= r1; x[3 * j + 2] -= r2; }
            if (a.tgt) store_pose<3>(a.tgt + item * 48, x);
            if (a.tgt_flip) { flip_pose<3>(x, y); store_pose<3>(a.tgt_flip + item * 48, y); }
        } else {
            const long long it2 = item - n3, i = it2 / a.F2;
            const int f = (int)(it2 - i * a.F2);
            const long long row = a.idx ? a.idx[i] : i, back = (i * a.F2 + (a.F2 - 1 - f)) * 32;
            float x[32], y[32];
            load_pose<2>(a.p2 + (row * a.F2 + f) * 32, x);
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

// ------------------------------------------------------------------------------------------------------------------ MSE
__global__ __launch_bounds__(kBlock) void pose_mse_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                          float* __restrict__ grad, long long n, float scale, int vec,
                                                          double* __restrict__ partials) {
    __shared__ double lds[4];
    double acc = 0.0;
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    const long long n4 = vec ? n >> 2 : 0;
    for (long long i = tid; i < n4; i += stride) {
        const float4 p = reinterpret_cast<const float4*>(pred)[i], t = reinterpret_cast<const float4*>(tgt)[i];
        const double d0 = (double)p.x - (double)t.x, d1 = (double)p.y - (double)t.y, d2 = (double)p.z - (double)t.z,
                     d3 = (double)p.w - (double)t.w;                                     // exact; (float) of it is the fp32 p - t
        acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
        reinterpret_cast<float4*>(grad)[i] = make_float4((float)d0 * scale, (float)d1 * scale, (float)d2 * scale, (float)d3 * scale);
    }
    for (long long i = 4 * n4 + tid; i < n; i += stride) {
        const double d = (double)pred[i] - (double)tgt[i];
        acc += d * d;
        grad[i] = (float)d * scale;
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// one wave: loss = fl32(sum / n), n = numel (MSE) or joints (MPJPE); the meter takes what AverageMeter.update(loss.item(), poses) adds
__global__ __launch_bounds__(64) void pose_mse_finish_kernel(const double* __restrict__ partials, int nparts, long long n,
                                                             long long poses, float* __restrict__ loss,
                                                             dhaug_loss_meter* __restrict__ meter) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 64) s += partials[b];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const float l = (float)(s / (double)n);
        *loss = l;
        if (meter) {
            meter->sum_loss_x_poses += (double)l * (double)poses;
            meter->poses += poses;
            meter->steps += 1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- MPJPE
// one joint: its distance (fp64), and d / (e * joints) rounded to fp32 once -- 0 where the distance is 0, NaN where it is NaN
__device__ __forceinline__ double mpjpe_joint(double dx, double dy, double dz, double joints, float& gx, float& gy, float& gz) {
    const double e = sqrt(dx * dx + dy * dy + dz * dz);
    const double den = e * joints;
    const bool zero = e == 0.0;
    gx = zero ? 0.0f : (float)(dx / den);
    gy = zero ? 0.0f : (float)(dy / den);
    gz = zero ? 0.0f : (float)(dz / den);
    return e;
}

__global__ __launch_bounds__(kBlock) void pose_mpjpe_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                            float* __restrict__ grad, long long joints, int vec,
                                                            double* __restrict__ partials) {
    __shared__ double lds[4];
    double acc = 0.0;
    const double nj = (double)joints;
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    const long long n4 = vec ? joints >> 2 : 0;                  // groups of four joints = 12 floats = three float4
    for (long long i = tid; i < n4; i += stride) {
        const float4* p4 = reinterpret_cast<const float4*>(pred) + 3 * i;
        const float4* t4 = reinterpret_cast<const float4*>(tgt) + 3 * i;
        const float4 p0 = p4[0], p1 = p4[1], p2 = p4[2], t0 = t4[0], t1 = t4[1], t2 = t4[2];
        float4 g0, g1, g2;
        acc += mpjpe_joint((double)p0.x - (double)t0.x, (double)p0.y - (double)t0.y, (double)p0.z - (double)t0.z, nj, g0.x, g0.y, g0.z);
        acc += mpjpe_joint((double)p0.w - (double)t0.w, (double)p1.x - (double)t1.x, (double)p1.y - (double)t1.y, nj, g0.w, g1.x, g1.y);
        acc += mpjpe_joint((double)p1.z - (double)t1.z, (double)p1.w - (double)t1.w, (double)p2.x - (double)t2.x, nj, g1.z, g1.w, g2.x);
        acc += mpjpe_joint((double)p2.y - (double)t2.y, (double)p2.z - (double)t2.z, (double)p2.w - (double)t2.w, nj, g2.y, g2.z, g2.w);
        float4* o4 = reinterpret_cast<float4*>(grad) + 3 * i;
        o4[0] = g0; o4[1] = g1; o4[2] = g2;
    }
    for (long long j = 4 * n4 + tid; j < joints; j += stride) {
        const float* p = pred + 3 * j;
        const float* t = tgt + 3 * j;
        float gx, gy, gz;
        acc += mpjpe_joint((double)p[0] - (double)t[0], (double)p[1] - (double)t[1], (double)p[2] - (double)t[2], nj, gx, gy, gz);
        grad[3 * j] = gx; grad[3 * j + 1] = gy; grad[3 * j + 2] = gz;
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------- gradient norm + Adam
// elements ahead of the first 16-byte boundary of p (0..3, at most n)
static inline long long head_of(const void* p, long long n) {
    const long long h = ((16 - (long long)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15) >> 2;
    return h < n ? h : n;
}

__global__ __launch_bounds__(kBlock) void grad_sumsq_kernel(const float* __restrict__ g, long long n, long long head,
                                                            float gscale, double* __restrict__ partials,
                                                            int* __restrict__ step_counter) {
    __shared__ double lds[4];
    double acc = 0.0;
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    const long long n4 = (n - head) >> 2;
    const float4* body = reinterpret_cast<const float4*>(g + head);
    for (long long i = tid; i < n4; i += stride) {
        const float4 v = body[i];
        const double a = (double)(v.x * gscale), b = (double)(v.y * gscale), c = (double)(v.z * gscale), d = (double)(v.w * gscale);
        acc += a * a; acc += b * b; acc += c * c; acc += d * d;
    }
    // the head ahead of the first whole float4 and the tail behind the last (at most three elements each)
    if (tid < head) {
        const double a = (double)(g[tid] * gscale);
        acc += a * a;
    }
    if (tid < n - head - 4 * n4) {
        const double a = (double)(g[head + 4 * n4 + tid] * gscale);
        acc += a * a;
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = acc;
        if (blockIdx.x == 0 && step_counter) *step_counter += 1;
    }
}

// Adam on an already scaled and clipped gradient gi (adam_dev_kernel's expressions, dhaug_elem.hip)
__device__ __forceinline__ float adam_update(float p, float gi, float& m, float& v, float lr, float b1, float b2, float eps,
                                             float bc1, float bc2_sqrt) {
    const float mi = m + (gi - m) * (1.0f - b1);
    const float vi = v * b2 + gi * gi * (1.0f - b2);
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    return p - (lr / bc1) * (mi / denom);
}
// the clipped gradient (g * grad_scale) * coef as a rounded fp32 value: the update cannot contract into it
__device__ __forceinline__ float clipped(float g, float gscale, float coef) {
    float gc = (g * gscale) * coef;
    asm volatile("" : "+v"(gc));
    return gc;
}

// LR_DEV = false: lr is the launch's immediate.  LR_DEV = true (dhaug_adam_clip_step_lr): every workgroup reads the one device float
// lr_dev, so a captured launch follows the schedule; everything after that load is the same statements.
template <bool LR_DEV>
__global__ __launch_bounds__(kBlock) void adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long long n, float lr_imm,
                                                           const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                           const int* __restrict__ step_dev, float gscale, float max_norm,
                                                           const double* __restrict__ partials, int nparts,
                                                           float* __restrict__ norm_out, int vec) {
    __shared__ double lds[4];
    const float lr = LR_DEV ? *lr_dev : lr_imm;
    double s = 0.0;
    for (int b = threadIdx.x; b < nparts; b += kBlock) s += partials[b];
    s = block_sum(s, lds);
    const float norm = (float)sqrt(s);
    const float c = max_norm / (norm + 1e-6f);
    const float coef = c > 1.0f ? 1.0f : c;                         // torch.clamp(c, max=1.0): a NaN stays a NaN
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = norm;
    const int step = *step_dev;
    const float bc1 = (float)(1.0 - pow((double)b1, (double)step)), bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    if (coef == 1.0f) {
        // (uniform) nothing to clip: adam_dev_kernel's loop statement for statement, so that the compiler contracts it the same way
        // (-ffp-contract=fast decides per expression shape) and the results are that kernel's bits
        for (long long i = tid; i < n; i += stride) {
            const float gi = g[i] * gscale;
            const float mi = m[i] + (gi - m[i]) * (1.0f - b1);
            const float vi = v[i] * b2 + gi * gi * (1.0f - b2);
            m[i] = mi;
            v[i] = vi;
            const float denom = sqrtf(vi) / bc2_sqrt + eps;
            p[i] = p[i] - (lr / bc1) * (mi / denom);
        }
        return;
    }
    const long long n4 = vec ? n >> 2 : 0;
    for (long long i = tid; i < n4; i += stride) {
        const float4 pv = reinterpret_cast<float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i], o;
        o.x = adam_update(pv.x, clipped(gv.x, gscale, coef), mv.x, vv.x, lr, b1, b2, eps, bc1, bc2_sqrt);
        o.y = adam_update(pv.y, clipped(gv.y, gscale, coef), mv.y, vv.y, lr, b1, b2, eps, bc1, bc2_sqrt);
        o.z = adam_update(pv.z, clipped(gv.z, gscale, coef), mv.z, vv.z, lr, b1, b2, eps, bc1, bc2_sqrt);
        o.w = adam_update(pv.w, clipped(gv.w, gscale, coef), mv.w, vv.w, lr, b1, b2, eps, bc1, bc2_sqrt);
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
        reinterpret_cast<float4*>(p)[i] = o;
    }
    for (long long i = 4 * n4 + tid; i < n; i += stride) {
        float mi = m[i], vi = v[i];
        const float o = adam_update(p[i], clipped(g[i], gscale, coef), mi, vi, lr, b1, b2, eps, bc1, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        p[i] = o;
    }
}

int sumsq_grid(int64_t n) { return dhaug_stream_grid((n + 3) / 4, kBlock, kSumsqMaxGrid); }

}  // namespace

extern "C" int dhaug_pair_batch(const float* p3, const float* p2, int64_t M, int F3, int F2, const int64_t* idx, int64_t n,
                                int flip, int playback, float* tgt, float* inp, float* tgt_flip, float* inp_flip,
                                float* inp_back, float* inp_flip_back, void* stream) {
    DHAUG_CHECK(n >= 0 && M >= 0 && F3 >= 1 && F2 >= 1, DHAUG_EINVAL);
    DHAUG_CHECK(idx != nullptr || n <= M, DHAUG_EINVAL);
    DHAUG_CHECK(flip || (!tgt_flip && !inp_flip && !inp_flip_back), DHAUG_EINVAL);
    DHAUG_CHECK(playback || (!inp_back && !inp_flip_back), DHAUG_EINVAL);
    const bool want3 = tgt || tgt_flip, want2 = inp || inp_flip || inp_back || inp_flip_back;
    DHAUG_CHECK(want3 || want2, DHAUG_EINVAL);
    DHAUG_CHECK((!want3 || p3) && (!want2 || p2), DHAUG_EINVAL);
    if (n == 0) return DHAUG_OK;
    const int Fmax = F3 > F2 ? F3 : F2;
    DHAUG_CHECK(n < (1ll << 31) / 48 / Fmax, DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(dhaug_aligned16(p3) && dhaug_aligned16(p2) && dhaug_aligned16(tgt) && dhaug_aligned16(inp) &&
                dhaug_aligned16(tgt_flip) && dhaug_aligned16(inp_flip) && dhaug_aligned16(inp_back) &&
                dhaug_aligned16(inp_flip_back) && (reinterpret_cast<uintptr_t>(idx) & 7u) == 0, DHAUG_EALIGN);
    PairArgs a;
    a.p3 = want3 ? p3 : nullptr; a.p2 = want2 ? p2 : nullptr;
    a.idx = reinterpret_cast<const long long*>(idx);
    a.tgt = tgt; a.tgt_flip = tgt_flip; a.inp = inp; a.inp_flip = inp_flip; a.inp_back = inp_back; a.inp_flip_back = inp_flip_back;
    a.n = n; a.F3 = F3; a.F2 = F2;
    const int64_t items = (want3 ? n * F3 : 0) + (want2 ? n * F2 : 0);
    hipLaunchKernelGGL(pair_batch_kernel, dim3(dhaug_stream_grid(items, kPairBlock, kMaxGrid)), dim3(kPairBlock), 0,
                       (hipStream_t)stream, a);
    return dhaug_launch_status();
}

extern "C" int dhaug_pose_mse(const float* pred, const float* tgt, int64_t numel, int64_t poses, float* grad, float* loss,
                              void* meter, void* workspace, void* stream) {
    DHAUG_CHECK(numel >= 0 && poses >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(grad != nullptr && loss != nullptr && workspace != nullptr, DHAUG_EINVAL);
    if (numel == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pred); DHAUG_CHECK_PTR(tgt);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt) | reinterpret_cast<uintptr_t>(grad) |
                 reinterpret_cast<uintptr_t>(loss)) % 4 == 0, DHAUG_EALIGN);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(meter)) % 8 == 0, DHAUG_EALIGN);
    const int vec = dhaug_aligned16(pred) && dhaug_aligned16(tgt) && dhaug_aligned16(grad);
    const int grid = dhaug_stream_grid((numel + 3) / 4, kBlock, kMaxGrid);
    const hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(pose_mse_kernel, dim3(grid), dim3(kBlock), 0, s, pred, tgt, grad, (long long)numel,
                       (float)(2.0 / (double)numel), vec, partials);
    hipLaunchKernelGGL(pose_mse_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)partials, grid, (long long)numel,
                       (long long)poses, loss, reinterpret_cast<dhaug_loss_meter*>(meter));
    return dhaug_launch_status();
}

extern "C" int dhaug_pose_mpjpe(const float* pred, const float* tgt, int64_t joints, int64_t poses, float* grad, float* loss,
                                void* meter, void* workspace, void* stream) {
    DHAUG_CHECK(joints >= 0 && poses >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(grad != nullptr && loss != nullptr && workspace != nullptr, DHAUG_EINVAL);
    if (joints == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pred); DHAUG_CHECK_PTR(tgt);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt) | reinterpret_cast<uintptr_t>(grad) |
                 reinterpret_cast<uintptr_t>(loss)) % 4 == 0, DHAUG_EALIGN);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(meter)) % 8 == 0, DHAUG_EALIGN);
    const int vec = dhaug_aligned16(pred) && dhaug_aligned16(tgt) && dhaug_aligned16(grad);
    const int grid = dhaug_stream_grid((joints + 3) / 4, kBlock, kMaxGrid);
    const hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(pose_mpjpe_kernel, dim3(grid), dim3(kBlock), 0, s, pred, tgt, grad, (long long)joints, vec, partials);
    hipLaunchKernelGGL(pose_mse_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)partials, grid, (long long)joints,
                       (long long)poses, loss, reinterpret_cast<dhaug_loss_meter*>(meter));
    return dhaug_launch_status();
}

extern "C" int dhaug_grad_sumsq(const float* grad, int64_t n, float grad_scale, void* workspace, int* step_counter,
                                void* stream) {
    DHAUG_CHECK(n >= 0 && workspace != nullptr, DHAUG_EINVAL);
    if (n == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(grad);
    DHAUG_CHECK(reinterpret_cast<uintptr_t>(grad) % 4 == 0 && reinterpret_cast<uintptr_t>(step_counter) % 4 == 0 &&
                reinterpret_cast<uintptr_t>(workspace) % 8 == 0, DHAUG_EALIGN);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(sumsq_grid(n)), dim3(kBlock), 0, (hipStream_t)stream, grad, (long long)n,
                       head_of(grad, n), grad_scale, reinterpret_cast<double*>(workspace), step_counter);
    return dhaug_launch_status();
}

namespace {

// dhaug_adam_clip_step and dhaug_adam_clip_step_lr: one set of checks, one launch shape
int adam_clip_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, const float* lr_dev,
                     bool from_dev, float beta1, float beta2, float eps, const int* step_dev, float grad_scale, float max_norm,
                     const void* workspace, float* norm_out, void* stream) {
    DHAUG_CHECK(n >= 0 && max_norm > 0.0f, DHAUG_EINVAL);                 // (a NaN max_norm fails the comparison)
    DHAUG_CHECK(step_dev != nullptr && workspace != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(!from_dev || lr_dev != nullptr, DHAUG_EINVAL);
    if (n == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(param); DHAUG_CHECK_PTR(grad); DHAUG_CHECK_PTR(exp_avg); DHAUG_CHECK_PTR(exp_avg_sq);
    DHAUG_CHECK((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
                 reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(step_dev) |
                 reinterpret_cast<uintptr_t>(norm_out) | reinterpret_cast<uintptr_t>(lr_dev)) % 4 == 0 &&
                reinterpret_cast<uintptr_t>(workspace) % 8 == 0, DHAUG_EALIGN);
    const int vec = dhaug_aligned16(param) && dhaug_aligned16(grad) && dhaug_aligned16(exp_avg) && dhaug_aligned16(exp_avg_sq);
    const dim3 grid(dhaug_stream_grid((n + 3) / 4, kBlock, kMaxGrid));
    if (from_dev)
        hipLaunchKernelGGL(adam_clip_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                           (long long)n, 0.0f, lr_dev, beta1, beta2, eps, step_dev, grad_scale, max_norm,
                           reinterpret_cast<const double*>(workspace), sumsq_grid(n), norm_out, vec);
    else
        hipLaunchKernelGGL(adam_clip_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                           (long long)n, lr, (const float*)nullptr, beta1, beta2, eps, step_dev, grad_scale, max_norm,
                           reinterpret_cast<const double*>(workspace), sumsq_grid(n), norm_out, vec);
    return dhaug_launch_status();
}

}  // namespace

extern "C" int dhaug_adam_clip_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                    float beta1, float beta2, float eps, const int* step_dev, float grad_scale, float max_norm,
                                    const void* workspace, float* norm_out, void* stream) {
    return adam_clip_launch(param, grad, exp_avg, exp_avg_sq, n, lr, nullptr, false, beta1, beta2, eps, step_dev, grad_scale, max_norm,
                            workspace, norm_out, stream);
}

extern "C" int dhaug_adam_clip_step_lr(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                       const float* lr_dev, float beta1, float beta2, float eps, const int* step_dev,
                                       float grad_scale, float max_norm, const void* workspace, float* norm_out, void* stream) {
    return adam_clip_launch(param, grad, exp_avg, exp_avg_sq, n, 0.0f, lr_dev, true, beta1, beta2, eps, step_dev, grad_scale, max_norm,
                            workspace, norm_out, stream);
}

namespace {

// *cell += value on a 64-bit cell (the dropout stream's base): one workgroup, one thread, a plain load, add and vector store
__global__ void u64_add_kernel(unsigned long long* cell, unsigned long long value) { *cell += value; }

}  // namespace

extern "C" int dhaug_u64_add(uint64_t* cell, uint64_t value, void* stream) {
    DHAUG_CHECK_PTR(cell);
    DHAUG_CHECK(reinterpret_cast<uintptr_t>(cell) % 8 == 0, DHAUG_EALIGN);
    hipLaunchKernelGGL(u64_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, reinterpret_cast<unsigned long long*>(cell),
                       (unsigned long long)value);
    return dhaug_launch_status();
}
