// Per-pose inverse kinematics of the DH skeleton: analytic Jacobian, closed-form bone lengths, Levenberg-Marquardt.
// Host and device compile the same source (tests/ikcheck builds it for the host under ASan + UBSan).
//
// Unknowns.  The generator drives 31 angle slots; six slots are pinned to 0 (4, 9, 22, 23, 28, 33: dhaug_fk_math.h kSlotCol).
// Of the 31, slots 27 and 32 turn a leaf frame and move no joint: their Jacobian columns, their rows of H = J^T J and their
// entries of g = J^T r are exact zeros, so (H + lambda diag(H) + eps I) delta = g gives them delta = 0 whatever the rest
// holds.  The solver therefore factors the other NU = 29 and leaves those two slots at their (clamped) start value, which
// is the same arithmetic for every other unknown.
//
// Jacobian.  With the chain frames of the forward walk (rotation axis z_k = column 2 of the cumulative frame C_k, pivot
// t_k = its origin) a joint p_j downstream of k moves by  d p_j / d theta_k = (pi/180) z_k x (p_j - t_k).  Everything is
// kept in the CHAIN frame (before the global rotation Rg): Rg is orthogonal, so J^T J and J^T r are the same there when r
// is turned back by Rg^T, and the three global angles become three more axes through the origin
//     x: Rg^T x^ = row 0 of Rg      y: Rg^T Rx y^      z: z^.
// alpha = +-90 deg is exact in these frames (EPS = false), as in fk_pose_backward.
//
// Normal equations.  H has arrow structure: a leg's angles move only that leg, the head's and an arm's angles only that
// limb, the nine body angles move head and arms, the global angles everything.  Ordering the unknowns
//     0..3 right leg | 4..7 left leg | 8..10 head | 11..13 right arm | 14..16 left arm | 17..25 body | 26..28 global
// puts every nonzero of the lower triangle inside the row profile first_of(i)..i, and Cholesky fills in nothing outside a
// profile: 248 floats instead of 435.  One lane owns one pose; H and g live in a workspace the caller hands over (LDS,
// one column per lane, on the device; a plain array on the host) and are walked by rolled loops whose indices are
// uniform; angles, frames and residuals are registers with compile-time indices.
#pragma once
#include "dhaug_fk_math.h"

namespace dhaug_ik {
using namespace dhaug_fk;

constexpr int NU = 29;                      // unknowns that move a joint
constexpr int U_BODY = 17, U_GLOBAL = 26;   // first body / global unknown
constexpr int H_FLOATS = 248;               // profile-packed lower triangle
constexpr int WS_FLOATS = H_FLOATS + NU;    // + g (then delta)
constexpr float kEpsDiag = 1e-8f;           // the eps of (H + lambda diag(H) + eps I): (m/deg)^2
constexpr float kLamMin = 1e-9f, kLamMax = 1e6f, kLamDown = 0.3f, kLamUp = 5.0f;

// angle slot of unknown u
DHAUG_HD constexpr int slot_of(int u) {
    constexpr int t[NU] = {0, 1, 2, 3, 5, 6, 7, 8, 19, 20, 21, 24, 25, 26, 29, 30, 31, 10, 11, 12, 13, 14, 15, 16, 17, 18, 34, 35, 36};
    return t[u];
}
// first column of row i's profile, and where the row starts in the packed array
DHAUG_HD constexpr int first_of(int i) {
    constexpr int t[NU] = {0, 0, 0, 0, 4, 4, 4, 4, 8, 8, 8, 11, 11, 11, 14, 14, 14, 8, 8, 8, 8, 8, 8, 8, 8, 8, 0, 0, 0};
    return t[i];
}
DHAUG_HD constexpr int row_of(int i) {
    constexpr int t[NU] = {0, 1, 3, 6, 10, 11, 13, 16, 20, 21, 23, 26, 27, 29, 32, 33, 35,
                           38, 48, 59, 71, 84, 98, 113, 129, 146, 164, 191, 219};
    return t[i];
}
DHAUG_HD constexpr int h_index(int i, int j) { return row_of(i) + j - first_of(i); }    // j in first_of(i)..i
static_assert(h_index(NU - 1, NU - 1) == H_FLOATS - 1, "profile");
// The same two tables as arithmetic, for the rolled loops of factor / solve: a table indexed at run time would be copied to
// scratch memory, a chain of selects on a uniform index is scalar code.  Rows b.. of one limb share the first column f,
// so row i starts (i - b)(b - f + 1) + (i - b)(i - b - 1) / 2 words behind row b.
DHAUG_HD constexpr int block_of(int i) { return i < 4 ? 0 : i < 8 ? 4 : i < 11 ? 8 : i < 14 ? 11 : i < 17 ? 14 : i < 26 ? 17 : 26; }
DHAUG_HD constexpr int first_rt(int i) { return i < 4 ? 0 : i < 8 ? 4 : i < 11 ? 8 : i < 14 ? 11 : i < 17 ? 14 : i < 26 ? 8 : 0; }
DHAUG_HD constexpr int row_rt(int i) {
    const int b = block_of(i), f = first_rt(i), d = i - b;
    const int rb = b == 0 ? 0 : b == 4 ? 10 : b == 8 ? 20 : b == 11 ? 26 : b == 14 ? 32 : b == 17 ? 38 : 164;
    return rb + d * (b - f + 1) + d * (d - 1) / 2;
}
DHAUG_HD constexpr bool tables_agree() {
    for (int i = 0; i < NU; ++i)
        if (first_rt(i) != first_of(i) || row_rt(i) != row_of(i)) return false;
    return true;
}
static_assert(tables_agree(), "first_rt / row_rt restate first_of / row_of");
DHAUG_HD constexpr bool dead_slot(int s) { return kSlotCol[s] < 0; }

// element e of this pose's workspace
struct Ws {
    float* p;
    int stride;
    DHAUG_HD float& operator()(int e) const { return p[(long)e * stride]; }
};

// ---- the unknowns that move joint J: its own limb's [O0, O1), the first NB body angles, the three global ones ----
template <int O0, int O1, int NB> DHAUG_HD constexpr int joint_unknowns() { return (O1 - O0) + NB + 3; }
template <int O0, int O1, int NB> DHAUG_HD constexpr int joint_unknown(int a) {
    return a < O1 - O0 ? O0 + a : (a < O1 - O0 + NB ? U_BODY + (a - (O1 - O0)) : U_GLOBAL + (a - (O1 - O0) - NB));
}

struct Frames { V3 Z[NU], T[NU]; };

template <int J, int O0, int O1, int NB, class Sink>
DHAUG_HD void emit_joint(const Frames& f, V3 q, const Rot& Rg, Sink& sink) {
    constexpr int n = joint_unknowns<O0, O1, NB>();
    V3 c[n];
#pragma unroll
    for (int a = 0; a < n; ++a) {
        const int u = joint_unknown<O0, O1, NB>(a);
        c[a] = kDeg2Rad * cross(f.Z[u], q - f.T[u]);
    }
    sink.template joint<J, O0, O1, NB>(c, q, Rg);
}

// Walks the skeleton at ang[37] / bl[15] (dead slots as given) and hands the sink, joint by joint, the chain-frame Jacobian
// columns of that joint with respect to the unknowns that move it.
template <class Sink>
DHAUG_HD void jacobian_walk(const float* __restrict__ ang, const float* __restrict__ bl, Sink& sink) {
    constexpr bool GUARD = true;
    float sgx, cgx;
    const Rot Rg = fk_global<GUARD>(ang, sgx, cgx);
    const V3 O = mk(0.0f, 0.0f, 0.0f);
    Frames f;
    f.Z[26] = Rg.r0;                                   f.T[26] = O;
    f.Z[27] = rot_apply_t(Rg, mk(0.0f, cgx, sgx));     f.T[27] = O;
    f.Z[28] = mk(0.0f, 0.0f, 1.0f);                    f.T[28] = O;
#define DHAUG_IK_CAPTURE(u) f.Z[u] = F.c2; f.T[u] = F.t
    {   // right leg
        DHAUG_SC(0, 0.0f); DHAUG_SC(1, -90.0f); DHAUG_SC(2, 180.0f); DHAUG_SC(3, 0.0f);
        Frame F = dh_first<0, false>(bl[5], 0.0f, s0, c0);                     DHAUG_IK_CAPTURE(0);
        emit_joint<1, 0, 0, 0>(f, F.t, Rg, sink);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s1, c1);        DHAUG_IK_CAPTURE(1);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s2, c2);        DHAUG_IK_CAPTURE(2);
        dh_apply<0, true, false, true, false>(F, bl[3], 0.0f, s3, c3);         DHAUG_IK_CAPTURE(3);
        emit_joint<2, 0, 3, 0>(f, F.t, Rg, sink);
        dh_apply<0, true, false, false, false>(F, bl[1], 0.0f, 0.0f, 1.0f);
        emit_joint<3, 0, 4, 0>(f, F.t, Rg, sink);
    }
    {   // left leg
        DHAUG_SC(5, 180.0f); DHAUG_SC(6, -90.0f); DHAUG_SC(7, 0.0f); DHAUG_SC(8, 0.0f);
        Frame F = dh_first<0, false>(-bl[4], 0.0f, s5, c5);                    DHAUG_IK_CAPTURE(4);
        emit_joint<4, 4, 4, 0>(f, F.t, Rg, sink);
        dh_apply<1, false, false, true, false>(F, 0.0f, 0.0f, s6, c6);         DHAUG_IK_CAPTURE(5);
        dh_apply<1, false, false, true, false>(F, 0.0f, 0.0f, s7, c7);         DHAUG_IK_CAPTURE(6);
        dh_apply<0, true, false, true, false>(F, bl[2], 0.0f, s8, c8);         DHAUG_IK_CAPTURE(7);
        emit_joint<5, 4, 7, 0>(f, F.t, Rg, sink);
        dh_apply<0, true, false, false, false>(F, bl[0], 0.0f, 0.0f, 1.0f);
        emit_joint<6, 4, 8, 0>(f, F.t, Rg, sink);
    }
    // body frames 0..8 = unknowns 17..25; Spine is the origin of frame 3, Thorax of frame 6
    DHAUG_SC(10, 90.0f); DHAUG_SC(11, -90.0f); DHAUG_SC(12, -90.0f); DHAUG_SC(13, -90.0f); DHAUG_SC(14, -90.0f);
    DHAUG_SC(15, -90.0f); DHAUG_SC(16, -90.0f); DHAUG_SC(17, -90.0f); DHAUG_SC(18, -90.0f);
    Frame B;
    {
        Frame F = dh_first<0, false>(0.0f, 0.0f, s10, c10);                    DHAUG_IK_CAPTURE(17);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s11, c11);      DHAUG_IK_CAPTURE(18);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s12, c12);      DHAUG_IK_CAPTURE(19);
        dh_apply<-1, false, true, true, false>(F, 0.0f, bl[6], s13, c13);      DHAUG_IK_CAPTURE(20);
        emit_joint<7, 0, 0, 3>(f, F.t, Rg, sink);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s14, c14);      DHAUG_IK_CAPTURE(21);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s15, c15);      DHAUG_IK_CAPTURE(22);
        dh_apply<-1, false, true, true, false>(F, 0.0f, bl[7], s16, c16);      DHAUG_IK_CAPTURE(23);
        emit_joint<8, 0, 0, 6>(f, F.t, Rg, sink);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s17, c17);      DHAUG_IK_CAPTURE(24);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s18, c18);      DHAUG_IK_CAPTURE(25);
        B = F;
    }
    {   // head
        DHAUG_SC(19, -90.0f); DHAUG_SC(20, -90.0f); DHAUG_SC(21, 0.0f);
        Frame F = B;
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s19, c19);      DHAUG_IK_CAPTURE(8);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s20, c20);      DHAUG_IK_CAPTURE(9);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s21, c21);      DHAUG_IK_CAPTURE(10);
        dh_apply<1, true, false, false, false>(F, bl[14], 0.0f, 0.0f, 1.0f);
        emit_joint<9, 8, 11, 9>(f, F.t, Rg, sink);
    }
    {   // right arm (slot 23 is pinned: no unknown)
        DHAUG_SC(23, -180.0f); DHAUG_SC(24, -90.0f); DHAUG_SC(25, 180.0f); DHAUG_SC(26, 0.0f);
        Frame F = B;
        dh_apply<-1, true, false, true, false>(F, -bl[9], 0.0f, s23, c23);
        emit_joint<13, 11, 11, 9>(f, F.t, Rg, sink);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s24, c24);      DHAUG_IK_CAPTURE(11);
        dh_apply<-1, false, false, true, false>(F, 0.0f, 0.0f, s25, c25);      DHAUG_IK_CAPTURE(12);
        dh_apply<0, true, false, true, false>(F, bl[11], 0.0f, s26, c26);      DHAUG_IK_CAPTURE(13);
        emit_joint<14, 11, 13, 9>(f, F.t, Rg, sink);
        dh_apply<0, true, false, false, false>(F, bl[13], 0.0f, 0.0f, 1.0f);
        emit_joint<15, 11, 14, 9>(f, F.t, Rg, sink);
    }
    {   // left arm (slot 28 is pinned)
        DHAUG_SC(28, 0.0f); DHAUG_SC(29, -90.0f); DHAUG_SC(30, 0.0f); DHAUG_SC(31, 0.0f);
        Frame F = B;
        dh_apply<-1, true, false, true, false>(F, bl[8], 0.0f, s28, c28);
        emit_joint<10, 14, 14, 9>(f, F.t, Rg, sink);
        dh_apply<1, false, false, true, false>(F, 0.0f, 0.0f, s29, c29);       DHAUG_IK_CAPTURE(14);
        dh_apply<1, false, false, true, false>(F, 0.0f, 0.0f, s30, c30);       DHAUG_IK_CAPTURE(15);
        dh_apply<0, true, false, true, false>(F, bl[10], 0.0f, s31, c31);      DHAUG_IK_CAPTURE(16);
        emit_joint<11, 14, 16, 9>(f, F.t, Rg, sink);
        dh_apply<0, true, false, false, false>(F, bl[12], 0.0f, 0.0f, 1.0f);
        emit_joint<12, 14, 17, 9>(f, F.t, Rg, sink);
    }
#undef DHAUG_IK_CAPTURE
}

// joint j of a target row (48 floats)
DHAUG_HD V3 target_joint(const float* __restrict__ pose, int j) { return mk(pose[3 * j], pose[3 * j + 1], pose[3 * j + 2]); }

// Sink of dhaug_fk_jacobian: world-frame columns into row-major J (48, 37), metres per degree.  The caller zeroed J.
struct JacobianStore {
    float* J;
    template <int JT, int O0, int O1, int NB>
    DHAUG_HD void joint(const V3* c, V3, const Rot& Rg) {
        constexpr int n = joint_unknowns<O0, O1, NB>();
#pragma unroll
        for (int a = 0; a < n; ++a) {
            const int s = slot_of(joint_unknown<O0, O1, NB>(a));
            const V3 w = rot_apply(Rg, c[a]);
            J[(3 * JT + 0) * 37 + s] = w.x;
            J[(3 * JT + 1) * 37 + s] = w.y;
            J[(3 * JT + 2) * 37 + s] = w.z;
        }
    }
};

// ---- per-joint weights of the residual: cost = sum_j w_j^2 |r_j|^2, H += w_j^2 c_a . c_b, g += w_j^2 c_a . h (joints 1..15; the
// root has no term).  A weight table is the same for every pose of a launch, so it never sits in a lane's registers: the
// device reads the squares from the kernel's arguments (scalar loads) and tests a bit mask for "w_j > 0" (which joints
// count for the reported residual).
// UnitWeights is dhaug_ik_fit / dhaug_ik_track: plain sums, nothing skipped.  JointWeights with every square 1.0f gives
// the same bits (fmaf(1, d, s) = s + d rounded once).
struct UnitWeights {
    DHAUG_HD constexpr bool on(int) const { return true; }
    DHAUG_HD float acc(int, float s, float d) const { return s + d; }
};
struct JointWeights {
    const float* w2;    // 16 squares (entry 0 unused)
    unsigned mask;      // bit j: w_j > 0
    DHAUG_HD bool on(int j) const { return (mask >> j) & 1u; }
    DHAUG_HD float acc(int j, float s, float d) const { return fmaf(w2[j], d, s); }
};

// Sink of the solver: H += c_a . c_b, g += c_a . (Rg^T r_J).  r_J is taken from the walk's own joint (alpha exact: 4e-8 of a
// bone length away from fk_pose's, below the rounding of a joint metres from the origin) so that no residual vector has to
// stay in registers through the walk; the accept / reject test uses fk_pose's cost (residual_cost).  A joint of weight 0
// adds exact zeros.  It is NOT branched around: a branch per joint splits the walk into basic blocks, the compiler then
// contracts a * b - c differently where the product and the difference land in different blocks, and one stage of weights
// 1 no longer gives fit_pose's bits (seen on gfx950).
template <class WT>
struct NormalEquations {
    Ws ws;
    const float* pose;
    V3 root;
    WT wt;
    template <int JT, int O0, int O1, int NB>
    DHAUG_HD void joint(const V3* c, V3 q, const Rot& Rg) {
        constexpr int n = joint_unknowns<O0, O1, NB>();
        const V3 h = rot_apply_t(Rg, (rot_apply(Rg, q) + root) - target_joint(pose, JT));
#pragma unroll
        for (int a = 0; a < n; ++a) {
            const int ua = joint_unknown<O0, O1, NB>(a);
            ws(H_FLOATS + ua) = wt.acc(JT, ws(H_FLOATS + ua), dot(c[a], h));
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                const int e = h_index(ua, joint_unknown<O0, O1, NB>(b));
                ws(e) = wt.acc(JT, ws(e), dot(c[a], c[b]));
            }
        }
    }
};

// In place: H + lambda diag(H) + eps I = L L^T inside the profile; the diagonal of L is stored inverted.
DHAUG_HD void factor(const Ws& ws, float lambda) {
    for (int i = 0; i < NU; ++i) {
        const int fi = first_rt(i), ri = row_rt(i) - fi;
        for (int j = fi; j <= i; ++j) {
            const int fj = first_rt(j), rj = row_rt(j) - fj;
            float s = ws(ri + j);
            if (j == i) s = fmaf(s, lambda, s) + kEpsDiag;
            for (int k = fi > fj ? fi : fj; k < j; ++k) s = fmaf(-ws(ri + k), ws(rj + k), s);
            // (rounding can push a pivot of a rank-deficient H below zero: the floor keeps the step finite, and the
            // accept / reject test then judges it like any other step)
            ws(ri + j) = j == i ? 1.0f / sqrtf(fmaxf(s, 1e-30f)) : s * ws(rj + j);
        }
    }
}
// g <- (L L^T)^-1 g
DHAUG_HD void solve(const Ws& ws) {
    for (int i = 0; i < NU; ++i) {
        const int fi = first_rt(i), ri = row_rt(i) - fi;
        float s = ws(H_FLOATS + i);
        for (int k = fi; k < i; ++k) s = fmaf(-ws(ri + k), ws(H_FLOATS + k), s);
        ws(H_FLOATS + i) = s * ws(ri + i);
    }
    for (int i = NU - 1; i >= 0; --i) {
        const int fi = first_rt(i), ri = row_rt(i) - fi;
        const float x = ws(H_FLOATS + i) * ws(ri + i);
        ws(H_FLOATS + i) = x;
        for (int k = fi; k < i; ++k) ws(H_FLOATS + k) = fmaf(-ws(ri + k), x, ws(H_FLOATS + k));
    }
}

DHAUG_HD float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// a - b as an unevaluated sum hi + lo (Knuth's two-sum: exact)
DHAUG_HD void diff2(float a, float b, float& hi, float& lo) {
    hi = a - b;
    const float bb = hi - a;
    lo = (a - (hi - bb)) + (-b - bb);
}
// The DH model's 15 lengths are the joint distances of used_16key_15bone_len_table.  |d|^2 carries the rounding error of
// the three differences (2 hi lo), which is what keeps the result within 2 ulp of the exact distance for joints metres
// away from the origin.
DHAUG_HD void bone_lengths(const V3* __restrict__ p, float* __restrict__ bl) {
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        const V3 a = p[kcs_bone_c(i)], b = p[kcs_bone_p(i)];
        float hx, lx, hy, ly, hz, lz;
        diff2(a.x, b.x, hx, lx); diff2(a.y, b.y, hy, ly); diff2(a.z, b.z, hz, lz);
        const float corr = 2.0f * fmaf(hz, lz, fmaf(hy, ly, hx * lx));
        bl[i] = sqrtf(fmaf(hz, hz, fmaf(hy, hy, fmaf(hx, hx, corr))));
    }
}

// sum over the joints of |FK16(ang, bl, root)_j - target_j|^2 with the joints as dhaug_fk_forward computes them (Hip = root: no
// term), each term times w_j^2, and the largest |r_j|^2 (unweighted) over the joints of weight > 0.  The target is read from
// the caller's row at every evaluation.
template <class WT>
DHAUG_HD float residual_cost(const float* __restrict__ ang, const float* __restrict__ bl, V3 root, const float* __restrict__ pose,
                             const WT& wt, float& worst) {
    V3 p[16];
    fk_pose<true>(ang, bl, p);
    float cost = 0.0f;
    worst = 0.0f;
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const V3 r = (p[j] + root) - target_joint(pose, j);
        const float d2 = dot(r, r);
        cost = wt.acc(j, cost, d2);
        worst = wt.on(j) ? fmaxf(worst, d2) : worst;
    }
    return cost;
}

// limits of slot s: the caller's tables (37 floats each) or the generator's
DHAUG_HD float limit_lo(const float* __restrict__ lo, int s) { return lo != nullptr ? lo[s] : kAngLo[s]; }
DHAUG_HD float limit_hi(const float* __restrict__ hi, int s) { return hi != nullptr ? hi[s] : kAngHi[s]; }

// What does not depend on the angles: root = joint 0, the 15 lengths (closed form, or bl_in where the caller has them), and the
// start clamped into the limits with the dead slots at 0.
DHAUG_HD void fit_start(const float* __restrict__ pose, const float* __restrict__ init, const float* __restrict__ lo,
                        const float* __restrict__ hi, const float* __restrict__ bl_in, float* __restrict__ ang,
                        float* __restrict__ bl, V3& root) {
    {
        V3 tgt[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) tgt[j] = target_joint(pose, j);
        root = tgt[0];
        if (bl_in == nullptr) {
            bone_lengths(tgt, bl);
        } else {
#pragma unroll
            for (int i = 0; i < 15; ++i) bl[i] = bl_in[i];
        }
    }
#pragma unroll
    for (int s = 0; s < 37; ++s)
        ang[s] = dead_slot(s) ? 0.0f : clampf(init != nullptr ? init[s] : 0.0f, limit_lo(lo, s), limit_hi(hi, s));
}

// `iters` Levenberg-Marquardt steps from ang (in place) under the weights wt, lambda starting at lambda0.  worst: the largest
// |r_j|^2 of where it ends, over the joints of weight > 0.
template <class WT>
DHAUG_HD void lm_steps(const float* __restrict__ pose, const float* __restrict__ lo, const float* __restrict__ hi, int iters,
                       float lambda0, const Ws& ws, const WT& wt, float* __restrict__ ang, const float* __restrict__ bl, V3 root,
                       float& worst) {
    float lambda = clampf(lambda0, kLamMin, kLamMax);
    float cost = residual_cost(ang, bl, root, pose, wt, worst);
    for (int it = 0; it < iters; ++it) {
        for (int e = 0; e < WS_FLOATS; ++e) ws(e) = 0.0f;
        {
            NormalEquations<WT> ne;
            ne.ws = ws; ne.pose = pose; ne.root = root; ne.wt = wt;
            jacobian_walk(ang, bl, ne);
        }
        factor(ws, lambda);
        solve(ws);
        float trial[37], worst2;
#pragma unroll
        for (int s = 0; s < 37; ++s) trial[s] = ang[s];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int s = slot_of(u);
            trial[s] = clampf(ang[s] - ws(H_FLOATS + u), limit_lo(lo, s), limit_hi(hi, s));
        }
        const float cost2 = residual_cost(trial, bl, root, pose, wt, worst2);
        const bool accept = cost2 < cost;
#pragma unroll
        for (int s = 0; s < 37; ++s) ang[s] = accept ? trial[s] : ang[s];
        cost = accept ? cost2 : cost;
        worst = accept ? worst2 : worst;
        lambda = clampf(lambda * (accept ? kLamDown : kLamUp), kLamMin, kLamMax);
    }
}

// One pose.  pose: the 48 floats of the target joints; init: 37 start angles or null (T-pose); lo / hi: 37 limits or null
// (kAngLo / kAngHi).  Writes ang[37] (dead slots 0), bl[15], root, residual (largest joint distance, metres).  Exactly
// `iters` Levenberg-Marquardt steps, no data-dependent exit.
DHAUG_HD void fit_pose(const float* __restrict__ pose, const float* __restrict__ init, const float* __restrict__ lo,
                       const float* __restrict__ hi, int iters, float lambda0, const Ws& ws, float* __restrict__ ang,
                       float* __restrict__ bl, V3& root, float& residual) {
    float worst;
    fit_start(pose, init, lo, hi, nullptr, ang, bl, root);
    lm_steps(pose, lo, hi, iters, lambda0, ws, UnitWeights(), ang, bl, root, worst);
    residual = sqrtf(worst);
}

// ---- coarse to fine: the same steps under one weight table per stage ----
constexpr int MAX_STAGES = 8;
// What a staged fit runs, by value: the device takes it as a kernel argument.  w2[s * 16 + j] = w_j^2 of stage s, mask[s] bit j
// = (w_j > 0), both for joints 1..15 (entry / bit 0 is not read: the root has no term).
struct StageTable {
    float w2[MAX_STAGES * 16];
    int iters[MAX_STAGES];
    unsigned mask[MAX_STAGES];
    int stages;
};
// Host: fills `t` from S rows of 16 weights and S step counts.  false (t undefined) for S outside 1..MAX_STAGES, a step
// count below 1, a weight that is negative or not finite, or a last stage without a joint of weight > 0.
inline bool make_stage_table(const float* weights, const int* iters, int S, StageTable& t) {
    if (weights == nullptr || iters == nullptr || S < 1 || S > MAX_STAGES) return false;
    t = StageTable();
    t.stages = S;
    for (int s = 0; s < S; ++s) {
        if (iters[s] < 1) return false;
        t.iters[s] = iters[s];
        for (int j = 0; j < 16; ++j) {
            const float w = weights[s * 16 + j];
            if (!(w >= 0.0f) || w > 3.0e38f) return false;      // (negative, NaN, inf)
            if (j == 0) continue;
            t.w2[s * 16 + j] = w * w;
            if (!(t.w2[s * 16 + j] <= 3.0e38f)) return false;   // (the square must be finite too)
            if (w > 0.0f) t.mask[s] |= 1u << j;
        }
    }
    return t.mask[S - 1] != 0;
}

// One pose, staged.  As fit_pose, but stage s = 0 .. stages - 1 runs iters[s] steps under that stage's weights from where
// the stage before stopped: lambda back at lambda0, the cost taken anew under the new weights.  bl_in: 15 lengths that
// replace the closed form, or null.  residual: the largest joint distance over the joints of weight > 0 in the LAST stage.
DHAUG_HD void fit_pose_staged(const float* __restrict__ pose, const float* __restrict__ init, const float* __restrict__ lo,
                              const float* __restrict__ hi, const float* __restrict__ bl_in, const StageTable& st, float lambda0,
                              const Ws& ws, float* __restrict__ ang, float* __restrict__ bl, V3& root, float& residual) {
    float worst = 0.0f;
    fit_start(pose, init, lo, hi, bl_in, ang, bl, root);
    for (int s = 0; s < st.stages; ++s) {
        JointWeights wt;
        wt.w2 = st.w2 + s * 16; wt.mask = st.mask[s];
        lm_steps(pose, lo, hi, st.iters[s], lambda0, ws, wt, ang, bl, root, worst);
    }
    residual = sqrtf(worst);
}

}  // namespace dhaug_ik
