// Posenet evaluation metrics (R/utils/loss.py: mpjpe, p_mpjpe :123-164, compute_PCK / compute_AUC :192-225, as
// R/function_aug/model_pos_eval.py:16-92 and R/models_Fk_GAN/video_mode_operate.py:769-876 call them): per pose of 16 joints,
// the joint errors, the PCK true positives at up to 32 thresholds and the P-MPJPE, plus a deterministic accumulation of
// their sums into a caller-owned device record.
//
// Layout: one pose per lane, 64-lane workgroups, a grid-stride loop over the poses.  A pose is 192 B per operand; a lane
// reads its own pose as 12 + 12 float4 loads (three passes: centroid, cross-covariance, aligned errors -- the second and
// third hit L1 / L2), so the fp64 3x3 solve runs on every lane, not on 1 lane of 16.  The reduction: every workgroup
// reduces its lanes' sums with a fixed xor butterfly and writes one partial record; a second one-wave launch adds the
// partials in workgroup order into the totals.  No atomics: the same call sequence gives bit-identical totals.
//
// Arithmetic:
//  * joint error (MPJPE and PCK) in fp32 as numpy evaluates compute_PCK's sqrt(sum(power(pred - gt, 2), 1)): d = p - g,
//    s = (dx*dx + dy*dy) + dz*dz with no contraction, correctly rounded sqrt; PCK compares fl32(e * 1000) < threshold.
//    A threshold held as fp64 is compared exactly: the host passes the smallest float >= threshold, and for a float v,
//    v < t  <=>  v < that float.
//  * P-MPJPE in fp64 from the fp32 inputs: centroids, S = sum (y - muY)(x - muX)^T, then the optimal proper rotation from
//    the dominant eigenvector of Horn's symmetric 4x4 matrix (cyclic Jacobi).  Its eigenvalue is s1 + s2 + sign * s3 of the
//    reference's sign-fixed SVD, so scale = lambda / |Y0|^2 and the aligned pose is scale * Q (y - muY) + muX.  A rank-1 or
//    rank-2 S has a repeated or zero eigenvalue: any eigenvector of the largest gives the same aligned points.  A pose with
//    zero spread (|X0| or |Y0| = 0) gives NaN, as the reference's 0 / 0 does.
#include "dhaug_common.h"

#include <math.h>

namespace {

constexpr int kBlock = 64;
constexpr int kMaxGrid = 2048;
constexpr int kPartialWords = 3 + DHAUG_EVAL_MAX_THRESHOLDS;   // sum_err, sum_pmpjpe (fp64 bits), poses, tp[32]

struct EvalArgs {
    const float* pred;
    const float* target;
    float* mpjpe;                 // (P,) or NULL
    float* pmpjpe;                // (P,) or NULL
    long long* partials;          // (gridDim.x, kPartialWords) or NULL (no totals)
    long long P;
    int center;
    int nthr;
    float cut[DHAUG_EVAL_MAX_THRESHOLDS];   // smallest float >= threshold; NaN past nthr (never true)
    int mult[16];
};

// fp32 joint error, evaluated exactly as numpy does it: no contraction, correctly rounded sqrt.  The build's
// -ffp-contract=fast lets the backend fuse any fmul + fadd whatever the source says (neither a contract(off) pragma nor
// __fmul_rn / __fadd_rn stop it), so every square passes through an empty asm the fusion cannot look through.
// __builtin_sqrtf is llvm.sqrt.f32 without !fpmath: the correctly rounded expansion (__fsqrt_rn may be the 1-ulp
// v_sqrt_f32 alone).
__device__ __forceinline__ float unfused(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ float joint_error_f32(float px, float py, float pz, float gx, float gy, float gz) {
    const float dx = px - gx, dy = py - gy, dz = pz - gz;
    const float s = (unfused(dx * dx) + unfused(dy * dy)) + unfused(dz * dz);
    return __builtin_sqrtf(s);
}

// one Jacobi rotation zeroing A[p][q] of the symmetric 4x4 A; V accumulates the eigenvectors (columns)
template <int p, int q>
__host__ __device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // inf theta -> t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq;
        A[k][q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk;
        A[q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

// S[a][b] = sum_j (y_j - muY)_a (x_j - muX)_b (y = prediction, x = target).  Returns the rotation Q (column-vector
// convention, Q (y - muY) ~ x - muX) and the dominant eigenvalue lambda = trace(Q S^T) = s1 + s2 + sign * s3.
__host__ __device__ __forceinline__ double optimal_rotation(const double (&S)[3][3], double (&Q)[3][3]) {
    const double sxx = S[0][0], sxy = S[0][1], sxz = S[0][2];
    const double syx = S[1][0], syy = S[1][1], syz = S[1][2];
    const double szx = S[2][0], szy = S[2][1], szz = S[2][2];
    double A[4][4] = {{sxx + syy + szz, syz - szy, szx - sxz, sxy - syx},
                      {syz - szy, sxx - syy - szz, sxy + syx, szx + sxz},
                      {szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy},
                      {sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] +
                           A[1][3] * A[1][3] + A[2][3] * A[2][3];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
        if (!(off > 1e-34 * diag)) break;          // converged (also stops on 0 / NaN)
        jacobi_rotate<0, 1>(A, V);
        jacobi_rotate<0, 2>(A, V);
        jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V);
        jacobi_rotate<1, 3>(A, V);
        jacobi_rotate<2, 3>(A, V);
    }
    // dominant eigenvector (the first of the largest eigenvalue), picked by 0 / 1 weights: a select between the columns of
    // V becomes a runtime-indexed load that sends V to scratch
    int best = 0;
    double lam = A[0][0];
    if (A[1][1] > lam) { best = 1; lam = A[1][1]; }
    if (A[2][2] > lam) { best = 2; lam = A[2][2]; }
    if (A[3][3] > lam) { best = 3; lam = A[3][3]; }
    const double w0 = best == 0, w1 = best == 1, w2 = best == 2, w3 = best == 3;
    const double q0 = V[0][0] * w0 + V[0][1] * w1 + V[0][2] * w2 + V[0][3] * w3;
    const double q1 = V[1][0] * w0 + V[1][1] * w1 + V[1][2] * w2 + V[1][3] * w3;
    const double q2 = V[2][0] * w0 + V[2][1] * w1 + V[2][2] * w2 + V[2][3] * w3;
    const double q3 = V[3][0] * w0 + V[3][1] * w1 + V[3][2] * w2 + V[3][3] * w3;
    const double inv = 1.0 / (q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    Q[0][0] = (q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3) * inv;
    Q[0][1] = 2.0 * (q1 * q2 - q0 * q3) * inv;
    Q[0][2] = 2.0 * (q1 * q3 + q0 * q2) * inv;
    Q[1][0] = 2.0 * (q1 * q2 + q0 * q3) * inv;
    Q[1][1] = (q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3) * inv;
    Q[1][2] = 2.0 * (q2 * q3 - q0 * q1) * inv;
    Q[2][0] = 2.0 * (q1 * q3 - q0 * q2) * inv;
    Q[2][1] = 2.0 * (q2 * q3 + q0 * q1) * inv;
    Q[2][2] = (q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3) * inv;
    return lam;
}

// joint j of a pose (16 x 3 fp32 at p), root-centred in fp32 when centring (x - x[:, :1], as the caller's torch code does)
struct Pose16 {
    const float4* v;
    float rx, ry, rz;
    __device__ __forceinline__ Pose16(const float* p, int center) : v(reinterpret_cast<const float4*>(p)) {
        const float4 r = v[0];
        rx = center ? r.x : 0.0f; ry = center ? r.y : 0.0f; rz = center ? r.z : 0.0f;
    }
    // a pass re-reads the pose (L1 / L2): an opaque copy of the pointer keeps the compiler from holding all 96 floats of
    // the first pass live across the solve
    __device__ __forceinline__ const float4* fresh() const {
        const float4* p = v;
        asm volatile("" : "+v"(p));
        return p;
    }
    // joints 4q..4q+3 (12 floats = 3 float4) through p = fresh()
    __device__ __forceinline__ void quad(const float4* p, int q, float (&o)[12]) const {
        const float4 a = p[3 * q], b = p[3 * q + 1], c = p[3 * q + 2];
        const float f[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 12; k += 3) {
            o[k] = f[k] - rx; o[k + 1] = f[k + 1] - ry; o[k + 2] = f[k + 2] - rz;
        }
    }
};

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kBlock);
    return v;
}

__global__ __launch_bounds__(kBlock) void pose_metrics_kernel(EvalArgs a) {
    double sum_err = 0.0, sum_p = 0.0;
    int poses = 0;
    int tp[DHAUG_EVAL_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) tp[k] = 0;

    for (long long n = (long long)blockIdx.x * kBlock + threadIdx.x; n < a.P; n += (long long)gridDim.x * kBlock) {
        const Pose16 Y(a.pred + n * 48, a.center), X(a.target + n * 48, a.center);
        // pass 1: fp32 joint errors, PCK counts, centroids
        double err = 0.0, my[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
        const float4 *yp = Y.fresh(), *xp = X.fresh();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float y[12], x[12];
            Y.quad(yp, q, y);
            X.quad(xp, q, x);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = 4 * q + jj;
                const float e = joint_error_f32(y[3 * jj], y[3 * jj + 1], y[3 * jj + 2], x[3 * jj], x[3 * jj + 1], x[3 * jj + 2]);
                err += (double)e;
                const float v = e * 1000.0f;
#pragma unroll
                for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) tp[k] += v < a.cut[k] ? a.mult[j] : 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    my[c] += (double)y[3 * jj + c];
                    mx[c] += (double)x[3 * jj + c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            my[c] *= 1.0 / 16.0;
            mx[c] *= 1.0 / 16.0;
        }
        // pass 2: cross-covariance and spreads of the centred poses
        double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, nx = 0.0, ny = 0.0;
        yp = Y.fresh(); xp = X.fresh();
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            float y[12], x[12];
            Y.quad(yp, q, y);
            X.quad(xp, q, x);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                double yc[3], xc[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    yc[c] = (double)y[3 * jj + c] - my[c];
                    xc[c] = (double)x[3 * jj + c] - mx[c];
                    ny += yc[c] * yc[c];
                    nx += xc[c] * xc[c];
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) S[r][c] += yc[r] * xc[c];
            }
        }
        double pm;
        if (!(nx > 0.0 && ny > 0.0)) {
            pm = __builtin_nan("");                   // the reference's 0 / 0 (a NaN spread stays NaN too)
        } else {
            double Q[3][3];
            const double scale = optimal_rotation(S, Q) / ny;
            // pass 3: aligned joint errors
            double acc = 0.0;
            yp = Y.fresh(); xp = X.fresh();
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                float y[12], x[12];
                Y.quad(yp, q, y);
                X.quad(xp, q, x);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    double yc[3], d2 = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) yc[c] = (double)y[3 * jj + c] - my[c];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const double d = scale * (Q[r][0] * yc[0] + Q[r][1] * yc[1] + Q[r][2] * yc[2]) -
                                         ((double)x[3 * jj + r] - mx[r]);
                        d2 += d * d;
                    }
                    acc += sqrt(d2);
                }
            }
            pm = acc * (1.0 / 16.0);
        }
        if (a.mpjpe) a.mpjpe[n] = (float)(err * (1.0 / 16.0));
        if (a.pmpjpe) a.pmpjpe[n] = (float)pm;
        sum_err += err;
        sum_p += pm;
        ++poses;
    }
    if (!a.partials) return;
    // workgroup partial: fixed xor butterfly over the wave (the workgroup is one wave)
    sum_err = wave_sum(sum_err);
    sum_p = wave_sum(sum_p);
    poses = wave_sum(poses);
    long long* out = a.partials + (long long)blockIdx.x * kPartialWords;
    if (threadIdx.x == 0) {
        out[0] = __builtin_bit_cast(long long, sum_err);
        out[1] = __builtin_bit_cast(long long, sum_p);
        out[2] = poses;
    }
#pragma unroll
    for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) {
        const int t = wave_sum(tp[k]);
        if (threadIdx.x == 0) out[3 + k] = t;
    }
}

// one wave: totals += sum over the partials, in workgroup order per lane, then a fixed butterfly
__global__ __launch_bounds__(kBlock) void pose_metrics_reduce_kernel(const long long* __restrict__ partials, int nparts,
                                                                     dhaug_eval_totals* __restrict__ tot) {
    double se = 0.0, sp = 0.0;
    long long n = 0, tp[DHAUG_EVAL_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) tp[k] = 0;
    for (int b = threadIdx.x; b < nparts; b += kBlock) {
        const long long* p = partials + (long long)b * kPartialWords;
        se += __builtin_bit_cast(double, p[0]);
        sp += __builtin_bit_cast(double, p[1]);
        n += p[2];
#pragma unroll
        for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) tp[k] += p[3 + k];
    }
    se = wave_sum(se);
    sp = wave_sum(sp);
    n = wave_sum(n);
#pragma unroll
    for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) tp[k] = wave_sum(tp[k]);
    if (threadIdx.x == 0) {
        tot->sum_err += se;
        tot->sum_pmpjpe += sp;
        tot->poses += n;
#pragma unroll
        for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) tot->tp[k] += tp[k];
    }
}

}  // namespace

extern "C" int dhaug_pose_metrics(const float* pred, const float* target, int64_t P, int center, const double* thresholds,
                                  int nthr, const int32_t* multiplicity, float* mpjpe_out, float* pmpjpe_out,
                                  void* totals, void* workspace, void* stream) {
    DHAUG_CHECK(P >= 0 && nthr >= 0 && nthr <= DHAUG_EVAL_MAX_THRESHOLDS, DHAUG_EINVAL);
    DHAUG_CHECK(nthr == 0 || thresholds != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(totals != nullptr || mpjpe_out != nullptr || pmpjpe_out != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(totals == nullptr || workspace != nullptr, DHAUG_EINVAL);
    EvalArgs a;
    for (int j = 0; j < 16; ++j) {
        const int m = multiplicity ? multiplicity[j] : 1;
        DHAUG_CHECK(m >= 0 && m <= DHAUG_EVAL_MAX_MULTIPLICITY, DHAUG_EINVAL);
        a.mult[j] = m;
    }
    for (int k = 0; k < DHAUG_EVAL_MAX_THRESHOLDS; ++k) {
        float c = __builtin_nanf("");
        if (k < nthr) {
            const double t = thresholds[k];
            c = (float)t;                                      // round to nearest, then up to the smallest float >= t
            if (!isnan(t) && (double)c < t) c = nextafterf(c, INFINITY);
        }
        a.cut[k] = c;
    }
    if (P == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pred); DHAUG_CHECK_PTR(target);
    // per-lane int32 PCK counters: at most 16 * 1024 * ceil(P / (2048 * 64)) per lane, < 2^31 for P < 2^31
    DHAUG_CHECK(P < (1ll << 31), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK(dhaug_aligned16(pred) && dhaug_aligned16(target), DHAUG_EALIGN);
    DHAUG_CHECK(totals == nullptr || ((uintptr_t)totals % 8 == 0 && (uintptr_t)workspace % 8 == 0), DHAUG_EALIGN);
    a.pred = pred; a.target = target;
    a.mpjpe = mpjpe_out; a.pmpjpe = pmpjpe_out;
    a.partials = reinterpret_cast<long long*>(workspace);
    if (!totals) a.partials = nullptr;
    a.P = P; a.center = center ? 1 : 0; a.nthr = nthr;
    const int grid = dhaug_stream_grid(P, kBlock, kMaxGrid);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_metrics_kernel, dim3(grid), dim3(kBlock), 0, s, a);
    if (totals) {
        hipLaunchKernelGGL(pose_metrics_reduce_kernel, dim3(1), dim3(kBlock), 0, s, (const long long*)a.partials, grid,
                           reinterpret_cast<dhaug_eval_totals*>(totals));
    }
    return dhaug_launch_status();
}
