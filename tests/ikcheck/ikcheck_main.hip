// TEST-ONLY stand-alone program: the per-pose inverse-kinematics arithmetic of csrc/dhaug_ik_math.h compiled for the HOST, so
// that it can run under AddressSanitizer + UBSan (tests/test_ik_cpu.py builds and runs it; nothing here is loaded into Python).
//
//   ikcheck [N = 64] [out.bin]
// draws N poses of the DH model (angles uniform in the middle 30 % of each generator range, default bone lengths +- 20 %,
// root (0.1, -0.2, 4.5)), starts each fit 5 degrees off per live slot, runs 12 Levenberg-Marquardt steps and prints one
// line per pose: "pose <i> residual <metres>".  With out.bin it also writes, as raw float32,
//   truth (N,37) | bone_len (N,15) | pose (N,48) | init (N,37) | angles (N,37) | fitted bone_len (N,15) | root (N,3) |
//   residual (N) | Jacobian at the truth (N,48,37)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dhaug_ik_math.h"

using namespace dhaug_ik;

namespace {
// (numerical recipes' 64-bit LCG: the draw only has to be spread out and the same on every run)
unsigned long long g_state = 0x2545F4914F6CDD1Dull;
float uniform01() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((g_state >> 40) & 0xFFFFFF) / 16777216.0f;
}
float uniform(float lo, float hi) { return lo + (hi - lo) * uniform01(); }
const float kDefaultLen[15] = {0.5f, 0.5f, 0.6f, 0.6f, 0.25f, 0.25f, 0.25f, 0.2f, 0.4f, 0.4f, 0.4f, 0.4f, 0.35f, 0.35f, 0.15f};
}  // namespace

int main(int argc, char** argv) {
    const long N = argc > 1 ? atol(argv[1]) : 64;
    if (N < 1 || N > (1 << 16)) return 2;
    std::vector<float> truth(N * 37), len(N * 15), pose(N * 48), init(N * 37), ang(N * 37), bl(N * 15), root(N * 3), res(N),
        J((size_t)N * 48 * 37, 0.0f), work(WS_FLOATS);
    for (long n = 0; n < N; ++n) {
        float* a = &truth[n * 37];
        for (int s = 0; s < 37; ++s) {
            const float mid = 0.5f * (kAngLo[s] + kAngHi[s]), half = 0.5f * (kAngHi[s] - kAngLo[s]);
            a[s] = dead_slot(s) ? 0.0f : uniform(mid - 0.3f * half, mid + 0.3f * half);
            init[n * 37 + s] = dead_slot(s) ? 0.0f : a[s] + uniform(-5.0f, 5.0f);
        }
        for (int i = 0; i < 15; ++i) len[n * 15 + i] = kDefaultLen[i] * uniform(0.8f, 1.2f);
        V3 p[16];
        fk_pose<true>(a, &len[n * 15], p);
        const V3 r = mk(0.1f, -0.2f, 4.5f);
        for (int j = 0; j < 16; ++j) {
            pose[n * 48 + 3 * j] = p[j].x + r.x; pose[n * 48 + 3 * j + 1] = p[j].y + r.y; pose[n * 48 + 3 * j + 2] = p[j].z + r.z;
        }
        Ws ws;
        ws.p = work.data(); ws.stride = 1;
        V3 rt;
        fit_pose(&pose[n * 48], &init[n * 37], nullptr, nullptr, 12, 1e-3f, ws, &ang[n * 37], &bl[n * 15], rt, res[n]);
        root[n * 3] = rt.x; root[n * 3 + 1] = rt.y; root[n * 3 + 2] = rt.z;
        JacobianStore sink;
        sink.J = &J[(size_t)n * 48 * 37];
        jacobian_walk(a, &len[n * 15], sink);
        printf("pose %ld residual %.9g\n", n, (double)res[n]);
    }
    if (argc > 2) {
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 3;
        for (const std::vector<float>* v : {&truth, &len, &pose, &init, &ang, &bl, &root, &res, &J}) fwrite(v->data(), 4, v->size(), o);
        fclose(o);
    }
    return 0;
}
