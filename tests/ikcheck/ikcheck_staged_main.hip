// TEST-ONLY stand-alone program: the staged, joint-weighted fit of csrc/dhaug_ik_math.h compiled for the HOST, so that it can
// run under AddressSanitizer + UBSan (tests/test_ik_staged_cpu.py builds and runs it; nothing here is loaded into Python).
//
//   ikcheck_staged [N = 64] [out.bin]
// draws N poses of the DH model as tests/ikcheck/ikcheck_main.hip does (angles uniform in the middle 30 % of each generator
// range, default bone lengths +- 20 %, root (0.1, -0.2, 4.5)) and fits each one COLD, from the T-pose, by the four-stage
// coarse-to-fine schedule (8 + 8 + 8 + 16 steps: joints {1,4,7} | + {8,10,13} | + {9,2,5,11,14} | all), once through
// fit_pose_staged and once stage by stage (fit_start, then lm_steps per stage) to see where every stage stops.  One line per
// pose: "pose <i> residual <metres>".  With out.bin it also writes, as raw float32,
//   truth (N,37) | bone_len (N,15) | pose (N,48) | stage weights (4,16) | angles after each stage (N,4,37) | angles (N,37) |
//   fitted bone_len (N,15) | root (N,3) | residual (N)
// It ends with status 4 if make_stage_table takes a table it must refuse.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "dhaug_ik_math.h"

using namespace dhaug_ik;

namespace {
unsigned long long g_state = 0x2545F4914F6CDD1Dull;
float uniform01() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((g_state >> 40) & 0xFFFFFF) / 16777216.0f;
}
float uniform(float lo, float hi) { return lo + (hi - lo) * uniform01(); }
const float kDefaultLen[15] = {0.5f, 0.5f, 0.6f, 0.6f, 0.25f, 0.25f, 0.25f, 0.2f, 0.4f, 0.4f, 0.4f, 0.4f, 0.35f, 0.35f, 0.15f};
constexpr int S = 4;
const int kStageJoints[S][16] = {{1, 4, 7, -1}, {1, 4, 7, 8, 10, 13, -1}, {1, 4, 7, 8, 10, 13, 9, 2, 5, 11, 14, -1},
                                 {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}};
const int kStageIters[S] = {8, 8, 8, 16};

bool refuses() {
    StageTable t;
    float w[9 * 16];
    int it[9];
    for (int i = 0; i < 9 * 16; ++i) w[i] = 1.0f;
    for (int i = 0; i < 9; ++i) it[i] = 1;
    if (!make_stage_table(w, it, 8, t) || make_stage_table(w, it, 0, t) || make_stage_table(w, it, 9, t)) return false;
    it[1] = 0;
    if (make_stage_table(w, it, 2, t)) return false;
    it[1] = 1;
    for (float bad : {-1.0f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(), 1e30f}) {
        w[5] = bad;
        if (make_stage_table(w, it, 1, t)) return false;
    }
    w[5] = 1.0f;
    for (int j = 1; j < 16; ++j) w[16 + j] = 0.0f;                 // a last stage of zeros (the root's entry does not count)
    return !make_stage_table(w, it, 2, t) && make_stage_table(w, it, 1, t);
}
}  // namespace

int main(int argc, char** argv) {
    const long N = argc > 1 ? atol(argv[1]) : 64;
    if (N < 1 || N > (1 << 16)) return 2;
    if (!refuses()) return 4;
    std::vector<float> weights(S * 16, 0.0f);
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < 16 && kStageJoints[s][k] >= 0; ++k) weights[s * 16 + kStageJoints[s][k]] = 1.0f;
    StageTable st;
    if (!make_stage_table(weights.data(), kStageIters, S, st)) return 4;
    std::vector<float> truth(N * 37), len(N * 15), pose(N * 48), stage_ang(N * S * 37), ang(N * 37), bl(N * 15), root(N * 3), res(N),
        work(WS_FLOATS);
    for (long n = 0; n < N; ++n) {
        float* a = &truth[n * 37];
        for (int s = 0; s < 37; ++s) {
            const float mid = 0.5f * (kAngLo[s] + kAngHi[s]), half = 0.5f * (kAngHi[s] - kAngLo[s]);
            a[s] = dead_slot(s) ? 0.0f : uniform(mid - 0.3f * half, mid + 0.3f * half);
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
        fit_pose_staged(&pose[n * 48], nullptr, nullptr, nullptr, nullptr, st, 1e-3f, ws, &ang[n * 37], &bl[n * 15], rt, res[n]);
        root[n * 3] = rt.x; root[n * 3 + 1] = rt.y; root[n * 3 + 2] = rt.z;
        {   // the same fit by hand, a stage at a time
            float cur[37], cur_bl[15], worst = 0.0f;
            V3 cur_rt;
            fit_start(&pose[n * 48], nullptr, nullptr, nullptr, nullptr, cur, cur_bl, cur_rt);
            for (int s = 0; s < S; ++s) {
                JointWeights wt;
                wt.w2 = st.w2 + s * 16; wt.mask = st.mask[s];
                lm_steps(&pose[n * 48], nullptr, nullptr, st.iters[s], 1e-3f, ws, wt, cur, cur_bl, cur_rt, worst);
                for (int k = 0; k < 37; ++k) stage_ang[(n * S + s) * 37 + k] = cur[k];
            }
        }
        printf("pose %ld residual %.9g\n", n, (double)res[n]);
    }
    if (argc > 2) {
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 3;
        for (const std::vector<float>* v : {&truth, &len, &pose, &weights, &stage_ang, &ang, &bl, &root, &res}) fwrite(v->data(), 4, v->size(), o);
        fclose(o);
    }
    return 0;
}
