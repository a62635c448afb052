// DOF angle distributions on the device: per-slot one-degree histograms, flags, exact extremes and fp64 moments of (rows, D)
// angle tables (dhaug_dof_histogram), and 361 x 361 joint tables of slot pairs (dhaug_dof_pair_histogram) -- what
// R/models_Fk_GAN/special_operate.py :347-364 and :420-442 build in Python loops.  The per-value arithmetic (bin, flags, the
// order of the extremes) is dhaug_dof_math.h; contract and record layout are in include/dhaug.h.
//
// dhaug_dof_histogram
//   Layout: a workgroup of 256 lanes, RG = 256 / D whole rows per step: lane l keeps slot l % D and reads row l / D of the
//   step, so a step is one contiguous stretch of RG * D floats (pitch = D) and a lane's slot -- and with it its extremes and
//   sums -- never changes.  Lanes RG * D .. 255 idle.  The rows are cut into slabs of consecutive steps, one workgroup each;
//   the partition depends on (rows, D) only (include/dhaug.h).
//   Integers: the bin counts go to an LDS table of D x 361 uint32 with no-return LDS adds (a slab has fewer than 2^31 rows, so
//   a counter cannot wrap); nan / outside / at_lo / at_hi / inf / skipped are lane registers added to small LDS counters once.  At
//   the end of the slab every NON-ZERO counter is added to the record's int64 word with a no-return global integer add.
//   Integer adds commute exactly: whatever order the workgroups arrive in, the words hold the same bits.
//   Floats: no atomic touches them.  The RG row-lanes of a slot meet in LDS in row order (extremes on the integer keys of
//   dhaug_dof_math.h, which makes them order-free anyway); the workgroup's (min, max, sum, sumsq) per slot go to the workspace,
//   and the second launch -- one workgroup -- adds the slabs' values in four interleaved chains per slot, the chains in order,
//   and then adds the result to the record.  That launch also adds `rows` to the record's row count.
//
// dhaug_dof_pair_histogram
//   One lane per row in a grid-stride loop; per pair two loads, two bins, one no-return global integer add.  Equal bins of a
//   wave are NOT folded into one add first: a saturated batch sends every add of a pair to one word (tools/time_dof.py
//   measures that case).
#include "dhaug_common.h"
#include "dhaug_dof_math.h"

namespace {

using namespace dhaug_dof;

constexpr int kBlock = DHAUG_DOF_BLOCK;
constexpr int kMaxBlocks = DHAUG_DOF_MAX_BLOCKS;
constexpr int kMinSteps = DHAUG_DOF_MIN_STEPS;
constexpr int kMaxSlots = DHAUG_DOF_MAX_SLOTS;
constexpr int kFoldChains = kBlock / kMaxSlots;               // 4 interleaved chains per slot in the second launch
constexpr int kMaxLdsBytes = kMaxSlots * kBins * 4;           // dynamic LDS of the histogram kernel at D = 64 (92 416 B)
constexpr int kPairMaxBlocks = 1024;

struct HistArgs {
    const float* angles;
    const float* residual;    // NULL: no row is skipped
    const float* lo;          // NULL (with hi): at_lo / at_hi are not counted
    const float* hi;
    unsigned long long* record;
    double* part;             // workspace: (slab, 4, kMaxSlots) min | max | sum | sumsq
    long long rows, pitch, slab_rows;
    float max_residual, tol;
    int D, rg;
};

// a row is kept when there is no residual, or residual <= max_residual (a NaN residual compares false: skipped)
__device__ __forceinline__ bool row_kept(const float* residual, long long r, float max_residual) {
    return residual == nullptr || residual[r] <= max_residual;
}

__device__ __forceinline__ void add_u64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: the no-return form
}

__global__ __launch_bounds__(kBlock) void dof_histogram_kernel(HistArgs a) {
    extern __shared__ unsigned int counts[];                  // (D, 361)
    __shared__ unsigned int flags_sm[5 * kMaxSlots];          // nan | outside | at_lo | at_hi | inf per slot
    __shared__ unsigned int skipped_sm;
    __shared__ int key_lo[kBlock], key_hi[kBlock];
    __shared__ double sum_sm[kBlock], sq_sm[kBlock];
    const int t = threadIdx.x, D = a.D;
    const int ncount = D * kBins;
    for (int i = t; i < ncount; i += kBlock) counts[i] = 0u;
    for (int i = t; i < 5 * kMaxSlots; i += kBlock) flags_sm[i] = 0u;
    if (t == 0) skipped_sm = 0u;
    __syncthreads();

    const int ro = t / D, d = t - ro * D;
    const long long begin = (long long)blockIdx.x * a.slab_rows;
    const long long end = begin + a.slab_rows < a.rows ? begin + a.slab_rows : a.rows;
    int kmin = 0x7fffffff, kmax = (int)0x80000000;            // above / below the key of every fp32 value
    double sum = 0.0, sq = 0.0;
    unsigned int n_nan = 0, n_out = 0, n_lo = 0, n_hi = 0, n_inf = 0, n_skip = 0;
    if (ro < a.rg) {
        const bool limits = a.lo != nullptr;
        const float lo_t = limits ? a.lo[d] + a.tol : 0.0f, hi_t = limits ? a.hi[d] - a.tol : 0.0f;
        unsigned int* my = counts + d * kBins;
        for (long long r = begin + ro; r < end; r += a.rg) {
            if (!row_kept(a.residual, r, a.max_residual)) {
                n_skip += d == 0 ? 1u : 0u;
                continue;
            }
            const float v = a.angles[r * a.pitch + d];
            int f;
            const int b = bin_of(v, f);
            if (f & F_NAN) {
                ++n_nan;
                continue;
            }
            (void)__hip_atomic_fetch_add(my + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            n_out += (f & F_OUTSIDE) ? 1u : 0u;
            const int k = order_key(v);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
            if (!(f & F_INF)) {
                const double x = (double)v;
                sum += x;
                sq += x * x;
            } else {
                ++n_inf;
            }
            if (limits) {
                n_lo += v <= lo_t ? 1u : 0u;
                n_hi += v >= hi_t ? 1u : 0u;
            }
        }
        if (n_nan) atomicAdd(&flags_sm[d], n_nan);
        if (n_out) atomicAdd(&flags_sm[kMaxSlots + d], n_out);
        if (n_lo) atomicAdd(&flags_sm[2 * kMaxSlots + d], n_lo);
        if (n_hi) atomicAdd(&flags_sm[3 * kMaxSlots + d], n_hi);
        if (n_inf) atomicAdd(&flags_sm[4 * kMaxSlots + d], n_inf);
        if (n_skip) atomicAdd(&skipped_sm, n_skip);
    }
    key_lo[t] = kmin; key_hi[t] = kmax;
    sum_sm[t] = sum; sq_sm[t] = sq;
    __syncthreads();

    // integers -> the record
    unsigned long long* rec = a.record;
    for (int i = t; i < ncount; i += kBlock) {
        const unsigned int c = counts[i];
        if (c) add_u64(rec + DHAUG_DOF_OFF_COUNTS(D) + i, c);
    }
    for (int i = t; i < 5 * D; i += kBlock) {
        const int which = i / D, s = i - which * D;            // nan | outside | at_lo | at_hi | inf: consecutive runs of D words
        const unsigned int c = flags_sm[which * kMaxSlots + s];
        if (c) add_u64(rec + DHAUG_DOF_OFF_NAN(D) + i, c);
    }
    if (t == 0 && skipped_sm) add_u64(rec + DHAUG_DOF_OFF_SKIPPED, skipped_sm);

    // floats -> the workspace: slot t, its row-lanes in row order
    if (t < D) {
        int lo_k = key_lo[t], hi_k = key_hi[t];
        double s = sum_sm[t], q = sq_sm[t];
        for (int k = 1; k < a.rg; ++k) {
            const int o = k * D + t;
            lo_k = key_lo[o] < lo_k ? key_lo[o] : lo_k;
            hi_k = key_hi[o] > hi_k ? key_hi[o] : hi_k;
            s += sum_sm[o];
            q += sq_sm[o];
        }
        double* out = a.part + (long long)blockIdx.x * 4 * kMaxSlots + t;
        // (an empty slab keeps the sentinels: +inf / -inf, the neutral elements of the fold)
        out[0] = lo_k == 0x7fffffff ? (double)INFINITY : (double)key_value(lo_k);
        out[kMaxSlots] = hi_k == (int)0x80000000 ? -(double)INFINITY : (double)key_value(hi_k);
        out[2 * kMaxSlots] = s;
        out[3 * kMaxSlots] = q;
    }
}

// min / max of two values that are fp32 numbers held in fp64 (or +-inf), by the keys of dhaug_dof_math.h
__device__ __forceinline__ double lower_of(double x, double y) { return order_key((float)y) < order_key((float)x) ? y : x; }
__device__ __forceinline__ double upper_of(double x, double y) { return order_key((float)y) > order_key((float)x) ? y : x; }

// one workgroup: record (min, max, sum, sumsq) <- record (op) the slabs' values, slab order; rows += rows
__global__ __launch_bounds__(kBlock) void dof_fold_kernel(const double* __restrict__ part, int slabs, int D, long long rows,
                                                          unsigned long long* __restrict__ record) {
    __shared__ double sm[4][kBlock];
    const int t = threadIdx.x, d = t % kMaxSlots, chain = t / kMaxSlots;
    double mn = (double)INFINITY, mx = -(double)INFINITY, s = 0.0, q = 0.0;
    if (d < D) {
        for (int b = chain; b < slabs; b += kFoldChains) {
            const double* p = part + (long long)b * 4 * kMaxSlots + d;
            mn = lower_of(mn, p[0]);
            mx = upper_of(mx, p[kMaxSlots]);
            s += p[2 * kMaxSlots];
            q += p[3 * kMaxSlots];
        }
    }
    sm[0][t] = mn; sm[1][t] = mx; sm[2][t] = s; sm[3][t] = q;
    __syncthreads();
    if (chain == 0 && d < D) {
        for (int c = 1; c < kFoldChains; ++c) {
            const int o = c * kMaxSlots + d;
            mn = lower_of(mn, sm[0][o]);
            mx = upper_of(mx, sm[1][o]);
            s += sm[2][o];
            q += sm[3][o];
        }
        double* f = reinterpret_cast<double*>(record);
        f[DHAUG_DOF_OFF_MIN(D) + d] = lower_of(f[DHAUG_DOF_OFF_MIN(D) + d], mn);
        f[DHAUG_DOF_OFF_MAX(D) + d] = upper_of(f[DHAUG_DOF_OFF_MAX(D) + d], mx);
        f[DHAUG_DOF_OFF_SUM(D) + d] += s;
        f[DHAUG_DOF_OFF_SUMSQ(D) + d] += q;
    }
    if (t == 0) record[DHAUG_DOF_OFF_ROWS] += (unsigned long long)rows;
}

struct PairArgs {
    const float* angles;
    const float* residual;
    unsigned long long* table;
    long long rows, pitch;
    float max_residual;
    int npairs;
    int slot[2 * DHAUG_DOF_MAX_PAIRS];
};

__global__ __launch_bounds__(kBlock) void dof_pair_kernel(PairArgs a) {
    for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < a.rows; r += (long long)gridDim.x * kBlock) {
        if (!row_kept(a.residual, r, a.max_residual)) continue;
        const float* row = a.angles + r * a.pitch;
#pragma unroll
        for (int p = 0; p < DHAUG_DOF_MAX_PAIRS; ++p) {
            if (p < a.npairs) {
                int fi, fj;
                const int bi = bin_of(row[a.slot[2 * p]], fi), bj = bin_of(row[a.slot[2 * p + 1]], fj);
                if (!((fi | fj) & F_NAN)) add_u64(a.table + ((long long)p * kBins + bi) * kBins + bj, 1ull);
            }
        }
    }
}

int check_common(const float* angles, int64_t rows, int64_t D, int64_t pitch) {
    DHAUG_CHECK(rows >= 0, DHAUG_EINVAL);
    DHAUG_CHECK(D >= 1 && D <= kMaxSlots, DHAUG_EINVAL);
    DHAUG_CHECK(pitch >= D, DHAUG_EINVAL);
    DHAUG_CHECK(rows == 0 || angles != nullptr, DHAUG_EINVAL);
    return DHAUG_OK;
}

}  // namespace

extern "C" int dhaug_dof_record_layout(int64_t D, int64_t* words13) {
    DHAUG_CHECK(D >= 1 && D <= kMaxSlots && words13 != nullptr, DHAUG_EINVAL);
    const int64_t w[13] = {DHAUG_DOF_OFF_ROWS, DHAUG_DOF_OFF_SKIPPED, DHAUG_DOF_OFF_NAN(D), DHAUG_DOF_OFF_OUTSIDE(D),
                           DHAUG_DOF_OFF_AT_LO(D), DHAUG_DOF_OFF_AT_HI(D), DHAUG_DOF_OFF_INF(D), DHAUG_DOF_OFF_MIN(D),
                           DHAUG_DOF_OFF_MAX(D), DHAUG_DOF_OFF_SUM(D), DHAUG_DOF_OFF_SUMSQ(D), DHAUG_DOF_OFF_COUNTS(D),
                           DHAUG_DOF_RECORD_WORDS(D)};
    for (int i = 0; i < 13; ++i) words13[i] = w[i];
    return DHAUG_OK;
}

extern "C" int dhaug_dof_histogram(const float* angles, int64_t rows, int64_t D, int64_t pitch, const float* residual,
                                   float max_residual, const float* lo, const float* hi, float tol, void* record, void* workspace,
                                   void* stream) {
    const int rc = check_common(angles, rows, D, pitch);
    if (rc != DHAUG_OK) return rc;
    DHAUG_CHECK(record != nullptr && workspace != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK((lo == nullptr) == (hi == nullptr), DHAUG_EINVAL);
    DHAUG_CHECK(rows < (1ll << 31), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK((uintptr_t)record % 8 == 0 && (uintptr_t)workspace % 8 == 0, DHAUG_EALIGN);
    if (rows == 0) return DHAUG_OK;
    HistArgs a;
    a.angles = angles; a.residual = residual; a.lo = lo; a.hi = hi;
    a.record = reinterpret_cast<unsigned long long*>(record);
    a.part = reinterpret_cast<double*>(workspace);
    a.rows = rows; a.pitch = pitch; a.max_residual = max_residual; a.tol = tol;
    a.D = (int)D; a.rg = kBlock / (int)D;
    const long long steps = (rows + a.rg - 1) / a.rg;
    long long slabs = (steps + kMinSteps - 1) / kMinSteps;
    if (slabs > kMaxBlocks) slabs = kMaxBlocks;
    const long long per = (steps + slabs - 1) / slabs;
    slabs = (steps + per - 1) / per;
    a.slab_rows = per * a.rg;
    const int lds = dhaug_dynamic_lds<dof_histogram_kernel>(kMaxLdsBytes);
    if (lds != DHAUG_OK) return lds;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dof_histogram_kernel, dim3((unsigned)slabs), dim3(kBlock), (size_t)a.D * kBins * 4, s, a);
    hipLaunchKernelGGL(dof_fold_kernel, dim3(1), dim3(kBlock), 0, s, (const double*)a.part, (int)slabs, a.D, (long long)rows,
                       a.record);
    return dhaug_launch_status();
}

extern "C" int dhaug_dof_pair_histogram(const float* angles, int64_t rows, int64_t D, int64_t pitch, const float* residual,
                                        float max_residual, const int* pairs, int npairs, int64_t* table, void* stream) {
    const int rc = check_common(angles, rows, D, pitch);
    if (rc != DHAUG_OK) return rc;
    DHAUG_CHECK(table != nullptr, DHAUG_EINVAL);
    DHAUG_CHECK(npairs >= 0 && npairs <= DHAUG_DOF_MAX_PAIRS, DHAUG_EINVAL);
    DHAUG_CHECK(npairs == 0 || pairs != nullptr, DHAUG_EINVAL);
    for (int i = 0; i < 2 * npairs; ++i) DHAUG_CHECK(pairs[i] >= 0 && pairs[i] < D, DHAUG_EINVAL);
    DHAUG_CHECK(rows < (1ll << 31), DHAUG_EUNSUPPORTED);
    DHAUG_CHECK((uintptr_t)table % 8 == 0, DHAUG_EALIGN);
    if (rows == 0 || npairs == 0) return DHAUG_OK;
    PairArgs a;
    a.angles = angles; a.residual = residual;
    a.table = reinterpret_cast<unsigned long long*>(table);
    a.rows = rows; a.pitch = pitch; a.max_residual = max_residual; a.npairs = npairs;
    for (int i = 0; i < 2 * DHAUG_DOF_MAX_PAIRS; ++i) a.slot[i] = i < 2 * npairs ? pairs[i] : 0;
    const int grid = dhaug_stream_grid(rows, kBlock, kPairMaxBlocks);
    hipLaunchKernelGGL(dof_pair_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    return dhaug_launch_status();
}
