// TEST-ONLY: runs the per-pose FK arithmetic of csrc/dhaug_fk_math.h on the HOST so that the container
// without a GPU can compare it with the oracle (tests/test_hostcheck_cpu.py), and exports the GEMM dispatchers' routing
// functions (csrc/dhaug_gemm_route.h).  Never loaded by the product.
#include "dhaug_fk_math.h"
#include "dhaug_gemm_route.h"
using namespace dhaug_fk;

extern "C" void hostcheck_fk_forward(const float* ang, const float* bl, const float* root, float* out16, long N) {
    for (long n = 0; n < N; ++n) {
        V3 p[16];
        fk_pose(ang + n * 37, bl + n * 15, p);
        for (int j = 0; j < 16; ++j) {
            out16[n * 48 + 3 * j + 0] = p[j].x + root[n * 3 + 0];
            out16[n * 48 + 3 * j + 1] = p[j].y + root[n * 3 + 1];
            out16[n * 48 + 3 * j + 2] = p[j].z + root[n * 3 + 2];
        }
    }
}

extern "C" void hostcheck_fk_backward(const float* ang, const float* bl, const float* g, float* gang, float* gbl,
                                      float* groot, long N) {
    for (long n = 0; n < N; ++n) {
        const float* mine = g + n * 48;
        V3 gr;
        fk_pose_backward(ang + n * 37, bl + n * 15,
                         [&](int j) { return mk(mine[3 * j], mine[3 * j + 1], mine[3 * j + 2]); },
                         gang + n * 37, gbl + n * 15, gr);
        groot[n * 3 + 0] = gr.x; groot[n * 3 + 1] = gr.y; groot[n * 3 + 2] = gr.z;
    }
}

extern "C" void hostcheck_tail_angles(const float* head, float* ang, float* root, long N, int preangle) {
    for (long n = 0; n < N; ++n) {
        float th[35];
        for (int c = 0; c < 35; ++c) th[c] = tanhf(head[n * 35 + c]);
        if (preangle) tail_angles<true>(th, ang + n * 37); else tail_angles<false>(th, ang + n * 37);
        for (int c = 0; c < 3; ++c) root[n * 3 + c] = th[32 + c] * 10.0f;
    }
}

extern "C" void hostcheck_sincos(const float* x, float* s, float* c, long N) {
    for (long n = 0; n < N; ++n) sincos_rad(x[n], s[n], c[n]);
}

// the generator tail's jitter draw: the Philox block function, the correctly rounded k / 1000, and one half of a pose's draw
extern "C" void hostcheck_philox4x32(const unsigned* counter4, const unsigned* key2, unsigned* out4, long n) {
    for (long i = 0; i < n; ++i) {
        unsigned r[4];
        philox4x32(counter4[4 * i], counter4[4 * i + 1], counter4[4 * i + 2], counter4[4 * i + 3], key2[2 * i], key2[2 * i + 1], r);
        for (int q = 0; q < 4; ++q) out4[4 * i + q] = r[q];
    }
}

extern "C" void hostcheck_div1000(const float* k, float* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = div1000(k[i]);
}

extern "C" void hostcheck_jitter(const unsigned long long* idx, unsigned long long seed, unsigned long long offset, float* out8, long n) {
    for (long i = 0; i < n; ++i) {
        jitter_half(idx[i], seed, offset, 0, out8 + 8 * i);
        jitter_half(idx[i], seed, offset, 1, out8 + 8 * i + 4);
    }
}

// the NT dispatcher's choice: 100 * dhaug_route::NtKernel + ksteps.  wide_min_tiles < 0: the default
extern "C" int hostcheck_nt_route(long long M, long long N, long long W, long long K, int out_bf16, int out_f32, int res_f32, int bias_ok,
                                  int mask_f32, int p8_ok, int no256, int nobig, int nop8, long long wide_min_tiles) {
    const dhaug_route::NtShape s{M, N, W, K, out_bf16 != 0, out_f32 != 0, res_f32 != 0, bias_ok != 0, mask_f32 != 0, p8_ok != 0,
                                 no256 != 0, nobig != 0, nop8 != 0, wide_min_tiles < 0 ? dhaug_route::WIDE_MIN_TILES_DEFAULT : wide_min_tiles};
    const dhaug_route::NtRoute r = dhaug_route::nt_route(s);
    return 100 * (int)r.kernel + r.ksteps;
}

extern "C" int hostcheck_tn_route(long long M, long long N1, long long N2) { return (int)dhaug_route::tn_route(M, N1, N2); }
