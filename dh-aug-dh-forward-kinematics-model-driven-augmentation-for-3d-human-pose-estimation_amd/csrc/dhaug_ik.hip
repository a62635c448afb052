// Inverse kinematics of the DH skeleton: analytic Jacobian, batched Levenberg-Marquardt fit, warm-started tracking.
//
// Mapping: one lane = one pose (ik_track: one sequence), one workgroup = one wave.  Poses do not talk to each other, so
// there is no barrier and no atomic anywhere; a lane's result depends on its own inputs only (same call, same bits).
// The solver's normal equations (profile-packed H, 248 floats, and g, 29 floats: dhaug_ik_math.h) sit in LDS, element e of
// lane l at word e * 64 + l: every access of a wave is one conflict-free row of 64 consecutive words and the element
// index is wave-uniform, so the rolled factor / solve loops address LDS without touching scratch.  277 x 64 x 4 B = 69.25 KB
// per wave: two waves per CU (160 KB), LDS is what bounds occupancy; the register budget of a lone wave on its SIMD (512)
// is what the fully unrolled Jacobian walk is compiled against.  Inputs and outputs move per lane (a pose is 192 B in,
// 224 B out against ~10^5 flops per iteration: the kernel is compute bound, the traffic is not staged through LDS).
#include "dhaug_ik_math.h"

using namespace dhaug_ik;

namespace {

constexpr int TILE = 64;
constexpr int IK_LDS_BYTES = WS_FLOATS * TILE * 4;

__device__ __forceinline__ void store_fit(long long n, const float* __restrict__ ang, const float* __restrict__ bl, V3 root,
                                          float residual, float* __restrict__ angles, float* __restrict__ bone_len,
                                          float* __restrict__ root_out, float* __restrict__ res_out) {
#pragma unroll
    for (int s = 0; s < 37; ++s) angles[n * 37 + s] = ang[s];
#pragma unroll
    for (int i = 0; i < 15; ++i) bone_len[n * 15 + i] = bl[i];
    root_out[n * 3] = root.x; root_out[n * 3 + 1] = root.y; root_out[n * 3 + 2] = root.z;
    res_out[n] = residual;
}

__global__ __launch_bounds__(TILE) void fk_jacobian_kernel(const float* __restrict__ angles, const float* __restrict__ bone_len,
                                                           float* __restrict__ J, long long N) {
    const long long ntiles = (N + TILE - 1) / TILE;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long n = tile * TILE + threadIdx.x;
        if (n >= N) continue;
        float ang[37], bl[15];
#pragma unroll
        for (int s = 0; s < 37; ++s) ang[s] = dead_slot(s) ? 0.0f : angles[n * 37 + s];
#pragma unroll
        for (int i = 0; i < 15; ++i) bl[i] = bone_len[n * 15 + i];
        JacobianStore sink;
        sink.J = J + n * (48 * 37);
        jacobian_walk(ang, bl, sink);
    }
}

__global__ __launch_bounds__(TILE) void ik_fit_kernel(const float* __restrict__ pose16, const float* __restrict__ init,
                                                      const float* __restrict__ lo, const float* __restrict__ hi,
                                                      float* __restrict__ angles, float* __restrict__ bone_len,
                                                      float* __restrict__ root_out, float* __restrict__ res_out, long long N,
                                                      int iters, float lambda0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x;
    Ws ws;
    ws.p = smem + lane; ws.stride = TILE;
    const long long ntiles = (N + TILE - 1) / TILE;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long n = tile * TILE + lane;
        const long long src = n < N ? n : N - 1;               // idle lanes of a ragged tile recompute the last pose (never stored)
        V3 root;
        float ang[37], bl[15], residual;
        fit_pose(pose16 + src * 48, init != nullptr ? init + src * 37 : nullptr, lo, hi, iters, lambda0, ws, ang, bl, root, residual);
        if (n < N) store_fit(n, ang, bl, root, residual, angles, bone_len, root_out, res_out);
    }
}

// ik_fit_kernel's layout; the stage table rides in the kernel's arguments (580 B), so a stage's weights are scalar loads
__global__ __launch_bounds__(TILE) void ik_fit_staged_kernel(const float* __restrict__ pose16, const float* __restrict__ init,
                                                             const float* __restrict__ lo, const float* __restrict__ hi,
                                                             const float* __restrict__ bone_len_in, const StageTable st,
                                                             float* __restrict__ angles, float* __restrict__ bone_len,
                                                             float* __restrict__ root_out, float* __restrict__ res_out, long long N,
                                                             float lambda0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x;
    Ws ws;
    ws.p = smem + lane; ws.stride = TILE;
    const long long ntiles = (N + TILE - 1) / TILE;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long n = tile * TILE + lane;
        const long long src = n < N ? n : N - 1;               // (idle lanes: as in ik_fit_kernel)
        V3 root;
        float ang[37], bl[15], residual;
        fit_pose_staged(pose16 + src * 48, init != nullptr ? init + src * 37 : nullptr, lo, hi,
                        bone_len_in != nullptr ? bone_len_in + src * 15 : nullptr, st, lambda0, ws, ang, bl, root, residual);
        if (n < N) store_fit(n, ang, bl, root, residual, angles, bone_len, root_out, res_out);
    }
}

// one lane per sequence: frame t starts from frame t - 1's angles
__global__ __launch_bounds__(TILE) void ik_track_kernel(const float* __restrict__ pose16, const long long* __restrict__ seq_offset,
                                                        const float* __restrict__ init, const float* __restrict__ lo,
                                                        const float* __restrict__ hi, float* __restrict__ angles,
                                                        float* __restrict__ bone_len, float* __restrict__ root_out,
                                                        float* __restrict__ res_out, long long S, int iters, float lambda0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x;
    Ws ws;
    ws.p = smem + lane; ws.stride = TILE;
    const long long ntiles = (S + TILE - 1) / TILE;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long s = tile * TILE + lane;
        if (s >= S) continue;                                   // (lanes share nothing: an idle lane may simply leave)
        const long long t0 = seq_offset[s], t1 = seq_offset[s + 1];
        float ang[37] = {}, bl[15], residual;
        V3 root;
        for (long long t = t0; t < t1; ++t) {
            // frame t0: the caller's start (or the T-pose); later frames: the row written one trip ago, read back in registers
            float start[37];
#pragma unroll
            for (int k = 0; k < 37; ++k) start[k] = t == t0 ? (init != nullptr ? init[s * 37 + k] : 0.0f) : ang[k];
            fit_pose(pose16 + t * 48, start, lo, hi, iters, lambda0, ws, ang, bl, root, residual);
            store_fit(t, ang, bl, root, residual, angles, bone_len, root_out, res_out);
        }
    }
}

template <auto Kern, typename... Args>
int launch_ik(long long items, void* stream, Args... args) {
    const int rc = dhaug_dynamic_lds<Kern>(IK_LDS_BYTES);
    if (rc != DHAUG_OK) return rc;
    const int grid = dhaug_stream_grid((items + TILE - 1) / TILE, 1, DHAUG_IK_MAX_BLOCKS);
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(TILE), IK_LDS_BYTES, (hipStream_t)stream, args...);
    return dhaug_launch_status();
}

}  // namespace

extern "C" {

int dhaug_fk_jacobian(const float* angles, const float* bone_len, float* J, int64_t N, void* stream) {
    DHAUG_CHECK(N >= 0, DHAUG_EINVAL);
    if (N == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(angles); DHAUG_CHECK_PTR(bone_len); DHAUG_CHECK_PTR(J);
    // the columns that are zero by structure (most of the matrix) are written once, by the fill; the kernel stores the rest
    const hipError_t e = hipMemsetAsync(J, 0, (size_t)N * 48 * 37 * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const int grid = dhaug_stream_grid((N + TILE - 1) / TILE, 1, DHAUG_FK_JACOBIAN_MAX_BLOCKS);
    hipLaunchKernelGGL(fk_jacobian_kernel, dim3(grid), dim3(TILE), 0, (hipStream_t)stream, angles, bone_len, J, (long long)N);
    return dhaug_launch_status();
}

int dhaug_ik_fit(const float* pose16, const float* init, const float* lo, const float* hi, float* angles, float* bone_len,
                 float* root, float* residual, int64_t N, int iters, float lambda0, void* stream) {
    DHAUG_CHECK(N >= 0 && iters >= 1 && lambda0 > 0.0f, DHAUG_EINVAL);
    DHAUG_CHECK((lo == nullptr) == (hi == nullptr), DHAUG_EINVAL);
    if (N == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pose16); DHAUG_CHECK_PTR(angles); DHAUG_CHECK_PTR(bone_len); DHAUG_CHECK_PTR(root); DHAUG_CHECK_PTR(residual);
    return launch_ik<ik_fit_kernel>(N, stream, pose16, init, lo, hi, angles, bone_len, root, residual, (long long)N, iters, lambda0);
}

int dhaug_ik_fit_staged(const float* pose16, const float* init, const float* lo, const float* hi, const float* bone_len_in,
                        const float* stage_weights, const int* stage_iters, int S, float lambda0, float* angles, float* bone_len,
                        float* root, float* residual, int64_t N, void* stream) {
    DHAUG_CHECK(N >= 0 && lambda0 > 0.0f, DHAUG_EINVAL);
    DHAUG_CHECK((lo == nullptr) == (hi == nullptr), DHAUG_EINVAL);
    StageTable st;
    DHAUG_CHECK(make_stage_table(stage_weights, stage_iters, S, st), DHAUG_EINVAL);
    if (N == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pose16); DHAUG_CHECK_PTR(angles); DHAUG_CHECK_PTR(bone_len); DHAUG_CHECK_PTR(root); DHAUG_CHECK_PTR(residual);
    return launch_ik<ik_fit_staged_kernel>(N, stream, pose16, init, lo, hi, bone_len_in, st, angles, bone_len, root, residual,
                                           (long long)N, lambda0);
}

int dhaug_ik_track(const float* pose16, const int64_t* seq_offset, const float* init, const float* lo, const float* hi,
                   float* angles, float* bone_len, float* root, float* residual, int64_t S, int iters, float lambda0,
                   void* stream) {
    DHAUG_CHECK(S >= 0 && iters >= 1 && lambda0 > 0.0f, DHAUG_EINVAL);
    DHAUG_CHECK((lo == nullptr) == (hi == nullptr), DHAUG_EINVAL);
    if (S == 0) return DHAUG_OK;
    DHAUG_CHECK_PTR(pose16); DHAUG_CHECK_PTR(seq_offset); DHAUG_CHECK_PTR(angles); DHAUG_CHECK_PTR(bone_len); DHAUG_CHECK_PTR(root);
    DHAUG_CHECK_PTR(residual);
    return launch_ik<ik_track_kernel>(S, stream, pose16, reinterpret_cast<const long long*>(seq_offset), init, lo, hi, angles,
                                      bone_len, root, residual, (long long)S, iters, lambda0);
}

}  // extern "C"
