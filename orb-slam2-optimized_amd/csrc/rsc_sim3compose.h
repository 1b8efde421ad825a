// rsc_sim3compose.h — the Sim3 bookkeeping between OptimizeSim3 and the loop MapPoint projection
// (src/LoopClosing.cpp:318-320), host arithmetic in IEEE double:
//     g2o::Sim3 gSmw(pKF->GetRotation().cast<double>(), pKF->GetTranslation().cast<double>(), 1.0);
//     mg2oScw = gScm * gSmw;
//     mScw = Converter::toIso(mg2oScw);
// * Sim3(Matrix3d, Vector3d, s) is r(Quaterniond(R)) with no normalisation (Thirdparty/g2o/g2o/types/sim3.h:64-67);
//   Quaterniond(R) follows Eigen 3.3's matrix-to-quaternion branches (po_quat_from_R, rsc_poseopt.h).
// * operator*: r = r1*r2; t = s1*(r1*t2)+t1; s = s1*s2 (sim3.h:266-272; so_mul, rsc_sim3opt.h).
// * toIso(Sim3) (src/Converter.cpp:31-37): linear() = rotation().toRotationMatrix().cast<float>() — the
//   unit rotation, NOT s*R — and translation() = translation().cast<float>(), not divided by s.
//
// Parity with the reference binary is UNPINNED for this part: Eigen's headers are not available to
// the build, as for g2o elsewhere.  The quaternion product follows Eigen's generic path
// (quat_product<Arch::Generic>); Eigen's SSE2 specialisation for doubles orders the same products
// differently and can differ in the last bit.  The trace and the quaternion-vector product sum left to
// right.  tests/kfproj_ref.py restates the same choices in numpy float64 and the two
// agree bit for bit.
#pragma once
#include "rsc_sim3opt.h"

namespace rsc {

// g2o::Sim3(R.cast<double>(), t.cast<double>(), 1.0) from a float pose (LoopClosing.cpp:318)
inline SoSim3 sc_sim3_from_pose(const float* R, const float* t) {
    double Rd[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rd[r][c] = (double)R[3 * r + c];
    SoSim3 S;
    S.r = po_quat_from_R(Rd);
    for (int c = 0; c < 3; ++c) S.t[c] = (double)t[c];
    S.s = 1.0;
    return S;
}

// q (x, y, z, w), t, s: the layout of rsc_loop_gate_result.S
inline SoSim3 sc_sim3_from_array(const double* S) {
    SoSim3 o;
    o.r.x = S[0]; o.r.y = S[1]; o.r.z = S[2]; o.r.w = S[3];
    o.t[0] = S[4]; o.t[1] = S[5]; o.t[2] = S[6];
    o.s = S[7];
    return o;
}

inline void sc_sim3_to_array(const SoSim3& a, double* S) {
    S[0] = a.r.x; S[1] = a.r.y; S[2] = a.r.z; S[3] = a.r.w;
    S[4] = a.t[0]; S[5] = a.t[1]; S[6] = a.t[2];
    S[7] = a.s;
}

// mg2oScw = gScm * gSmw (LoopClosing.cpp:319)
inline SoSim3 sc_compose(const SoSim3& gScm, const SoSim3& gSmw) { return so_mul(gScm, gSmw); }

// Converter::toIso(const g2o::Sim3&): row-major 4x4, last row 0 0 0 1
inline void sc_to_iso(const SoSim3& S, float* T) {
    double R[3][3];
    po_quat_to_R(S.r, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[r][c];
        T[4 * r + 3] = (float)S.t[r];
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

}  // namespace rsc
