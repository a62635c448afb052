// The detailed pose errors of R/utils/loss.py: mpjpe_byjoint :17-23, weighted_mpjpe :26-32, n_mpjpe :167-177 and
// mean_velocity_error :180-189, as two reductions with the conventions of dhaug_pose_metrics (dhaug_eval.hip): sums go
// into caller-zeroed device doubles, every workgroup writes fp64 partials to a caller workspace, a small second launch adds
// them in a fixed order.  No atomics: the same call sequence gives the same bits.
//
// dhaug_pose_column_errors -- (rows, cols, 3): per column c the sum over the rows of the joint error, and the sum over
// all row pairs (r, r + 1) and columns of the velocity error.
//   Layout: a lane owns a quad of 4 columns (12 floats = 3 float4 per operand).  With Q = cols / 4 quads per row, a
//   workgroup of 256 lanes covers RG = max(1, 256 / Q) whole consecutive rows per step when Q <= 256 (lane t: row t / Q of
//   the step, quad t % Q), and one 256-quad chunk of one row when Q > 256 (CC = ceil(Q / 256) chunks): either way the lanes
//   of a wave read one contiguous stretch of memory.  The rows are cut into slabs of consecutive steps, one workgroup per
//   (slab, chunk); a lane walks its slab downwards, RG rows per step, so its quad -- and its four column sums -- never change.
//   The velocity needs row r + 1 next to row r: with RG = 1 it is the lane's own next step and is carried in registers, so
//   every element is read once apart from one row per slab boundary; with RG > 1 another lane of the same workgroup reads it
//   in the same step (or the next), and the second read is a cache hit.
//   The partition depends on (rows, cols) only: steps = ceil(rows / RG), slabs = min(MAX_BLOCKS / CC, ceil(steps /
//   MIN_STEPS)), steps per slab = ceil(steps / slabs).
//   Reduction: column sums across the RG row-lanes of a workgroup in LDS, in row order; the workgroup's velocity sum by a
//   fixed butterfly per wave, then the 4 waves in order.  Second launch: a workgroup per 16 columns adds the slabs' partials
//   (16 interleaved chains, then those in order), one more workgroup adds the velocity partials.
//
// dhaug_pose_scaled_errors -- P poses (16, 3): the same quads, 4 lanes per pose and 64 poses per workgroup in a grid-stride
// loop; a pose's two dot products (sum t.p, sum p.p) meet in a two-level butterfly over its 4 lanes, so every element is read
// once and stays in registers for |s p - t| and w |p - t|.
//
// Arithmetic: root-centring (optional) in fp32 as dhaug_pose_metrics does it; everything after it in fp64 from the fp32
// values -- differences, squares, square roots, sums.
#include "dhaug_common.h"

#include <math.h>

namespace {

constexpr int kColBlock = 256;                  // lanes, and quads per chunk
constexpr int kColMaxBlocks = DHAUG_COLERR_MAX_BLOCKS;
constexpr int kColMinSteps = DHAUG_COLERR_MIN_STEPS;
constexpr int kRedCols = 16;                    // columns per workgroup of the second launch
constexpr int kRedChains = kColBlock / kRedCols;

constexpr int kPoseBlock = 64;                  // poses per workgroup (4 lanes each), and lanes of the one-wave reduction
constexpr int kPoseMaxGrid = DHAUG_SCALEDERR_MAX_BLOCKS;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// sum over the 256 lanes of a workgroup, valid in lane 0: a butterfly per wave, then the 4 waves in order
__device__ __forceinline__ double block_sum(double v, double* sm4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm4[0] + sm4[1]) + sm4[2]) + sm4[3];
}

// 4 joints (12 fp32) of one operand, minus the root when centring (fp32)
struct Quad {
    float f[12];
    __device__ __forceinline__ void load(const float* row, int q, int center) {
        const float4* p = reinterpret_cast<const float4*>(row) + 3 * (long long)q;
        const float4 a = p[0], b = p[1], c = p[2];
        const float v[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        float rx = 0.0f, ry = 0.0f, rz = 0.0f;
        if (center) {                             // the first joint of the quad's group of 16 joints (same or previous line)
            const float4 r = reinterpret_cast<const float4*>(row)[3 * (long long)(q & ~3)];
            rx = r.x; ry = r.y; rz = r.z;
        }
#pragma unroll
        for (int k = 0; k < 12; k += 3) {
            f[k] = center ? v[k] - rx : v[k];
            f[k + 1] = center ? v[k + 1] - ry : v[k + 1];
            f[k + 2] = center ? v[k + 2] - rz : v[k + 2];
        }
    }
};

struct ColArgs {
    const float* pred;
    const float* target;
    double* col_part;        // (slabs, cols)
    double* vel_part;        // (gridDim.x,)
    long long rows;
    long long slab_rows;     // rows per slab (a multiple of rg)
    int cols, Q, Qc, rg, cc, center;
};

template <bool COL, bool VEL>
__global__ __launch_bounds__(kColBlock) void column_errors_kernel(ColArgs a) {
    __shared__ double sm[kColBlock * 4];
    __shared__ double sm4[4];
    const int t = threadIdx.x;
    const int slab = blockIdx.x / a.cc, chunk = blockIdx.x % a.cc;
    const int ro = t / a.Qc, q = chunk * kColBlock + t % a.Qc;
    const long long begin = slab * a.slab_rows;
    const long long end = begin + a.slab_rows < a.rows ? begin + a.slab_rows : a.rows;
    const long long ld = 3ll * a.cols;
    double col[4] = {0.0, 0.0, 0.0, 0.0}, vel = 0.0;
    if (ro < a.rg && q < a.Q) {
        Quad pc, tc, pn, tn;
        bool carried = false;
        for (long long r = begin + ro; r < end; r += a.rg) {
            if (!carried) {
                pc.load(a.pred + r * ld, q, a.center);
                tc.load(a.target + r * ld, q, a.center);
            }
            carried = false;
            if (COL) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double dx = (double)pc.f[3 * j] - (double)tc.f[3 * j];
                    const double dy = (double)pc.f[3 * j + 1] - (double)tc.f[3 * j + 1];
                    const double dz = (double)pc.f[3 * j + 2] - (double)tc.f[3 * j + 2];
                    col[j] += sqrt(dx * dx + dy * dy + dz * dz);
                }
            }
            if (VEL && r + 1 < a.rows) {
                pn.load(a.pred + (r + 1) * ld, q, a.center);
                tn.load(a.target + (r + 1) * ld, q, a.center);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int k = 3 * j + c;
                        const double d = ((double)pn.f[k] - (double)pc.f[k]) - ((double)tn.f[k] - (double)tc.f[k]);
                        s += d * d;
                    }
                    vel += sqrt(s);
                }
                if (a.rg == 1) {                  // row r + 1 is this lane's next step
                    pc = pn; tc = tn;
                    carried = true;
                }
            }
        }
    }
    if (COL) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sm[4 * t + j] = col[j];
        __syncthreads();
        if (ro == 0 && q < a.Q) {
            double* out = a.col_part + (long long)slab * a.cols + 4ll * q;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
                for (int k = 0; k < a.rg; ++k) s += sm[4 * (k * a.Qc + t) + j];
                out[j] = s;
            }
        }
    }
    if (VEL) {
        const double v = block_sum(vel, sm4);
        if (t == 0) a.vel_part[blockIdx.x] = v;
    }
}

// workgroups 0 .. col_blocks - 1: col_sums[c] += the slabs' partials of 16 columns; workgroup col_blocks: *vel_sum += the
// workgroups' velocity partials
__global__ __launch_bounds__(kColBlock) void column_errors_reduce_kernel(const double* __restrict__ col_part,
                                                                         const double* __restrict__ vel_part, int slabs, int cols,
                                                                         int nblocks, int col_blocks, double* __restrict__ col_sums,
                                                                         double* __restrict__ vel_sum) {
    __shared__ double sm[kColBlock];
    __shared__ double sm4[4];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < col_blocks) {
        const int c = blockIdx.x * kRedCols + t % kRedCols, k = t / kRedCols;
        double s = 0.0;
        if (c < cols)
            for (int b = k; b < slabs; b += kRedChains) s += col_part[(long long)b * cols + c];
        sm[t] = s;
        __syncthreads();
        if (k == 0 && c < cols) {
            double tot = 0.0;
#pragma unroll
            for (int i = 0; i < kRedChains; ++i) tot += sm[i * kRedCols + t];
            col_sums[c] += tot;
        }
    } else {
        double s = 0.0;
        for (int b = t; b < nblocks; b += kColBlock) s += vel_part[b];
        s = block_sum(s, sm4);
        if (t == 0) *vel_sum += s;
    }
}

struct ScaledArgs {
    const float* pred;
    const float* target;
    const float* w;          // NULL, (P,) or (P, 16)
    double* partials;        // (gridDim.x, 2)
    long long P;
    int center, w_per_joint;
};

// A lane owns 4 joints of a pose (a Quad, as in the column kernel), 4 lanes a pose, a workgroup of 256 lanes 64 poses: a wave
// reads 16 whole poses as one contiguous stretch and every element once.  The two dot products of the scale are summed as a
// tree -- a joint's 3 products, the lane's 4 joints in pairs, the pose's 4 lanes by a two-level xor butterfly (every lane of the
// pose gets the same bits): at most 7 roundings on any path, whatever the 48 terms are (tests/eval_detail_util.py derives its
// bound from that).  The loop runs the same number of times in every lane of the workgroup, so the butterfly never meets an
// idle lane.
__global__ __launch_bounds__(kColBlock) void scaled_errors_kernel(ScaledArgs a) {
    __shared__ double sm4[4];
    const int t = threadIdx.x, q = t & 3;
    double sum_n = 0.0, sum_w = 0.0;
    for (long long base = (long long)blockIdx.x * kPoseBlock; base < a.P; base += (long long)gridDim.x * kPoseBlock) {
        const long long n = base + (t >> 2);
        const bool valid = n < a.P;
        Quad y, x;
#pragma unroll
        for (int k = 0; k < 12; ++k) y.f[k] = x.f[k] = 0.0f;
        float wj[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) {
            y.load(a.pred + n * 48, q, a.center);
            x.load(a.target + n * 48, q, a.center);
            if (a.w && a.w_per_joint) {
                const float4 w4 = reinterpret_cast<const float4*>(a.w + n * 16)[q];
                wj[0] = w4.x; wj[1] = w4.y; wj[2] = w4.z; wj[3] = w4.w;
            } else if (a.w) {
                wj[0] = wj[1] = wj[2] = wj[3] = a.w[n];
            }
        }
        // the scale s = sum t.p / sum p.p (the reference's two means over the joints cancel their 1 / 16)
        double tj[4], pj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double y0 = y.f[3 * j], y1 = y.f[3 * j + 1], y2 = y.f[3 * j + 2];
            tj[j] = (double)x.f[3 * j] * y0 + (double)x.f[3 * j + 1] * y1 + (double)x.f[3 * j + 2] * y2;
            pj[j] = y0 * y0 + y1 * y1 + y2 * y2;
        }
        double tp = (tj[0] + tj[1]) + (tj[2] + tj[3]), pp = (pj[0] + pj[1]) + (pj[2] + pj[3]);
        tp += __shfl_xor(tp, 1, 64); pp += __shfl_xor(pp, 1, 64);
        tp += __shfl_xor(tp, 2, 64); pp += __shfl_xor(pp, 2, 64);
        const double s = tp / pp;                                  // 0 / 0 = NaN, as the reference
        double en = 0.0, ew = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double d2 = 0.0, s2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double yy = (double)y.f[3 * j + c], xx = (double)x.f[3 * j + c];
                const double d = yy - xx, ds = s * yy - xx;
                d2 += d * d;
                s2 += ds * ds;
            }
            en += sqrt(s2);
            if (a.w) ew += (double)wj[j] * sqrt(d2);
        }
        if (valid) {
            sum_n += en;
            sum_w += ew;
        }
    }
    sum_n = block_sum(sum_n, sm4);
    __syncthreads();
    sum_w = block_sum(sum_w, sm4);
    if (t == 0) {
        a.partials[2ll * blockIdx.x] = sum_n;
        a.partials[2ll * blockIdx.x + 1] = sum_w;
    }
}

// one wave: sums += the partials, in workgroup order per lane, then a fixed butterfly
__global__ __launch_bounds__(kPoseBlock) void scaled_errors_reduce_kernel(const double* __restrict__ partials, int nparts,
                                                                         int weighted, double* __restrict__ sums) {
    double sn = 0.0, sw = 0.0;
    for (int b = threadIdx.x; b < nparts; b += kPoseBlock) {
        sn += partials[2 * b];
        sw += partials[2 * b + 1];
    }
    sn = wave_sum(sn);
    sw = wave_sum(sw);
    if (threadIdx.x == 0) {
        sums[0] += sn;
        if (weighted) sums[1] += sw;
    }
}

}  // namespace

extern "C" int dhaug_pose_column_errors(const float* pred, const float* target, int64_t rows, int64_t cols, int center,
                                        double* col_sums, double* vel_sum, void* workspace, void* stream) {
    DHAUG_CHECK(rows >= 0 && cols >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(col_sums != nullptr || vel_sum != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(workspace != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(!center || cols % 16 == 0, DHAUG_EINVAL);
    DHAUG_CHECK(cols <= DHAUG_COLERR_MAX_COLS && cols % 4 == 0 && rows < (1ll << 31), DHAUG_EUNSUPPORTED);
    if (rows == 0 || cols == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pred); DHAUG_CHECK_PTR(target);
    DHAUG_CHECK(dhaug_aligned16(pred) && dhaug_aligned16(target), DHAUG_EALIGN);
    DHAUG_CHECK((uintptr_t)col_sums % 8 == 0 && (uintptr_t)vel_sum % 8 == 0 && (uintptr_t)workspace % 8 == 0, DHAUG_EALIGN);
    if (!col_sums && rows == 1) return DHAUG_OK;                  // no row pair: vel_sum stays as it is
    ColArgs a;
    a.pred = pred; a.target = target;
    a.rows = rows; a.cols = (int)cols; a.center = center ? 1 : 0;
    a.Q = (int)cols / 4;
    a.Qc = a.Q < kColBlock ? a.Q : kColBlock;
    a.rg = kColBlock / a.Qc;
    a.cc = (a.Q + kColBlock - 1) / kColBlock;
    if (a.cc > 1) a.rg = 1;
    const long long steps = (rows + a.rg - 1) / a.rg;
    long long slabs = (steps + kColMinSteps - 1) / kColMinSteps;
    if (slabs > kColMaxBlocks / a.cc) slabs = kColMaxBlocks / a.cc;
    const long long per = (steps + slabs - 1) / slabs;
    slabs = (steps + per - 1) / per;
    a.slab_rows = per * a.rg;
    const int grid = (int)slabs * a.cc;
    a.vel_part = reinterpret_cast<double*>(workspace);
    a.col_part = a.vel_part + kColMaxBlocks;
    const hipStream_t s = (hipStream_t)stream;
    const bool vel = vel_sum != nullptr && rows > 1;
    if (col_sums && vel) hipLaunchKernelGGL((column_errors_kernel<true, true>), dim3(grid), dim3(kColBlock), 0, s, a);
    else if (col_sums) hipLaunchKernelGGL((column_errors_kernel<true, false>), dim3(grid), dim3(kColBlock), 0, s, a);
    else hipLaunchKernelGGL((column_errors_kernel<false, true>), dim3(grid), dim3(kColBlock), 0, s, a);
    const int col_blocks = col_sums ? ((int)cols + kRedCols - 1) / kRedCols : 0;
    hipLaunchKernelGGL(column_errors_reduce_kernel, dim3(col_blocks + (vel ? 1 : 0)), dim3(kColBlock), 0, s,
                       (const double*)a.col_part, (const double*)a.vel_part, (int)slabs, (int)cols, grid, col_blocks, col_sums,
                       vel_sum);
    return dhaug_launch_status();
}

extern "C" int dhaug_pose_scaled_errors(const float* pred, const float* target, int64_t P, int center, const float* w,
                                        int w_per_joint, double* sums, void* workspace, void* stream) {
    DHAUG_CHECK(P >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(sums != nullptr && workspace != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(P < (1ll << 31), DHAUG_EUNSUPPORTED);
    if (P == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pred); DHAUG_CHECK_PTR(target);
    DHAUG_CHECK(dhaug_aligned16(pred) && dhaug_aligned16(target), DHAUG_EALIGN);
    DHAUG_CHECK((uintptr_t)w % (w_per_joint ? 16 : 4) == 0, DHAUG_EALIGN);
    DHAUG_CHECK((uintptr_t)sums % 8 == 0 && (uintptr_t)workspace % 8 == 0, DHAUG_EALIGN);
    ScaledArgs a;
    a.pred = pred; a.target = target; a.w = w;
    a.partials = reinterpret_cast<double*>(workspace);
    a.P = P; a.center = center ? 1 : 0; a.w_per_joint = w_per_joint ? 1 : 0;
    const int grid = dhaug_stream_grid(P, kPoseBlock, kPoseMaxGrid);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(scaled_errors_kernel, dim3(grid), dim3(kColBlock), 0, s, a);
    hipLaunchKernelGGL(scaled_errors_reduce_kernel, dim3(1), dim3(kPoseBlock), 0, s, (const double*)a.partials, grid,
                       w != nullptr ? 1 : 0, sums);
    return dhaug_launch_status();
}
