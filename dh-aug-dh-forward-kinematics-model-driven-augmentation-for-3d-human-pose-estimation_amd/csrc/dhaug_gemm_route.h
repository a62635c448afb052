// Which kernel a GEMM takes: the whole decision of dhaug_gemm.hip's two dispatchers (gemm_bf16_impl for the NT products,
// dhaug_gemm_tn_bf16_rows for the TN products) as pure functions of the shape.  Plain C++ without HIP types, so the rules are
// pinned on the host (tests/test_cpu_boundary.py::test_gemm_routes through tests/hostcheck).  The dispatchers validate, read the
// environment switches ONCE, call these, and launch; nothing here reads the environment.
#pragma once

namespace dhaug_route {

// tile constants the thresholds below share with the kernels of dhaug_gemm.hip
constexpr int W_BM = 256, W_BN = 256;   // output tile of gemm_nt_wide_kernel (and of the ping-pong kernel, dhaug_gemm_p8.hip)
constexpr int F_BM = 64;                // gemm_nt256s_kernel: the batch is whole 64-row tiles (two of its 32-row tiles)
constexpr int TN_BN = 64;               // output tile edge of the TN kernels
constexpr int TF_ROWS = 128;            // gemm_tn64_kernel: contraction rows per stage

enum NtKernel { NT256S, WS, P8, WIDE, BIG, PIPE2, GENERIC_128x128, GENERIC_128x64, GENERIC_128x32 };
enum TnKernel { TN64, TN_GENERIC };

// what the NT choice depends on, and nothing else.  (The leading dimensions are not here: the dispatcher has checked
// lda >= K and ldb >= K, so K >= 64 covers the 64-column rows the staged copies of p8 / wide / big / pipe2 read.)
struct NtShape {
    long long M, N, W, K;               // W: output width covered by tiles (N, or the zero-padded width)
    bool out_bf16, out_f32;             // which outputs are present
    bool res_f32;                       // an fp32 residual is present
    bool bias_ok;                       // no bias, or a 16-byte aligned one
    bool mask_f32;                      // the activation-backward mask comes as fp32 values
    bool p8_ok;                         // dhaug_p8_supported() of the filled arguments
    // the switches (tests use them as cross-checks)
    bool no256, nobig, nop8;            // DHAUG_GEMM_NO256, DHAUG_GEMM_NOBIG, DHAUG_GEMM_NOP8
    long long wide_min_tiles;           // DHAUG_GEMM_WIDE_MIN_TILES, default 160
};
constexpr long long WIDE_MIN_TILES_DEFAULT = 160;

struct NtRoute {
    NtKernel kernel;
    int ksteps;                         // K / 16: the template argument of NT256S (8, 16) and WS (1, 2, 3, 4, 7, 8, 16); else 0
};

inline NtRoute nt_route(const NtShape& s) {
    const int ks = (int)(s.K / 16);
    // the training path's 256-wide layers: bf16 in, bf16 out
    if (!s.mask_f32 && s.N == 256 && s.W == 256 && s.M % F_BM == 0 && s.out_bf16 && !s.out_f32 && !s.res_f32 && s.bias_ok && !s.no256 &&
        (s.K == 128 || s.K == 256))
        return {NT256S, ks};
    // weight-stationary: every K / 16 the kernel is instantiated for
    if (!s.mask_f32 && s.W > 64 && s.K <= 256 && (ks == 1 || ks == 2 || ks == 3 || ks == 4 || ks == 7 || ks == 8 || ks == 16)) return {WS, ks};
    const bool staged = s.K >= 64;      // kernels whose copies read whole 64-column rows of both operands
    // long batch, tiles enough for most of the card: 256 x 256 tiles, eight waves (the DenseDim-1000 layers of the frame critics;
    // the 256-wide layers of the split-operand parity arithmetic, K' = 3 K or 6 K) -- the ping-pong kernel where it takes the
    // problem, else the five-stage kernel
    if (staged && !s.nobig && s.W >= 256 && ((s.M + W_BM - 1) / W_BM) * ((s.W + W_BN - 1) / W_BN) >= s.wide_min_tiles)
        return {s.p8_ok && !s.nop8 ? P8 : WIDE, 0};
    // long batch, wide layer: 128 x 256 tiles, 64 x 128 per wave
    if (staged && !s.nobig && s.W >= 512 && s.M >= 4096) return {BIG, 0};
    if (staged && s.W > 64) return {PIPE2, 0};
    return {s.W > 64 ? GENERIC_128x128 : s.W > 32 ? GENERIC_128x64 : GENERIC_128x32, 0};
}

// gemm_tn64_kernel copies whole 128-row stages (so M % 128 == 0, at least four of them); ragged N1 / N2 cost it zero-filled
// chunks, which pays from sixteen stages on
inline TnKernel tn_route(long long M, long long N1, long long N2) {
    const bool whole = N1 % TN_BN == 0 && N2 % TN_BN == 0;
    return (whole || M >= 16 * TF_ROWS) && M % TF_ROWS == 0 && M >= 4 * TF_ROWS ? TN64 : TN_GENERIC;
}

}  // namespace dhaug_route
