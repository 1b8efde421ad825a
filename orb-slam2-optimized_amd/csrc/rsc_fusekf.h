// rsc_fusekf.h — ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cpp:671-821), the matcher of
// LocalMapping::SearchInNeighbors (src/LocalMapping.cpp:433-510): device layout and the arithmetic of one
// (point, KeyFrame) pair, shared by fusekf.hip and the host emulation (tests/fusekf_emu).
//
// No coupling between the points of a call: bestIdx is read (:790-794) before any bookkeeping (:798-817) and
// no keypoint is ever skipped, so every pair is decided alone and the bookkeeping (Replace, AddObservation,
// AddMapPoint) is the caller's, replayed in list order (facade/ORBmatcher.hpp).
//
// What differs from the Sim3 Fuse (kfp_setup(fuse = true), kfp_fuse_point), kept as the reference has it:
//   pose       Rcw, tcw are the KeyFrame's own (:673-674); Ow is GetCameraCenter(), the stored
//              Twc.translation() (KeyFrame.cpp:57-66,85-89), read from the view, never recomputed as -R^T t
//   invz       1/p3Dc.z() is a float division (:705), not the double division of :865
//   ur         u - bf*invz (:716), read by the stereo branch only
//   keypoint   mvuRight[idx] >= 0 is stereo (:760), +0 and -0 included: not the `> 0` of proj_stereo_gate
//   stereo     e2 = (ex*ex+ey*ey)+er*er in float, rejected when (double)(e2*invSigma2[kpLevel]) > 7.8 (:769-771)
//   mono       e2 = ex*ex+ey*ey, rejected when (double)(e2*invSigma2[kpLevel]) > 5.99 (:780-782)
//   invSigma2  mvInvLevelSigma2[l] = 1.0f/(sf[l]*sf[l]) as ORBextractor.cpp:359,367 derives it from
//              mvScaleFactors: float multiply, IEEE float divide, no contraction
// What is the same: z < 0 skips (z == +-0 gives inf / NaN, IsInImage is false); u = fx*(x*invz)+cx; IsInImage
// excludes the maximum; 0.8f*dmin <= dist3D <= 1.2f*dmax; PO.dot(Pn) < 0.5*dist3D in double; PredictScale
// clamped to [0, n_levels); GetFeaturesInArea's strict window; octave in [L-1, L]; bestDist starts at 256 under
// a strict < in visiting order (proj_walk's order is the tie-break), kept when <= TH_LOW.
//
// fkf_setup restates kfp_setup's gates rather than calling it: kfp_setup derives Ow from R and t and does not
// return invz, and the kernels built on it keep their code as it is.
//
// Precondition (checked by rsc_fuse_kf_many): every keypoint octave of the KeyFrame is in [0, n_levels).
#pragma once
#include "rsc_kfproj.h"

namespace rsc {

constexpr double kFkfChi2Stereo = 7.8, kFkfChi2Mono = 5.99;  // :771, :782

struct FuseKfProblem {
    DevKfpKF K;
    DevKfpPoints P;
    float Rcw[9], tcw[3];    // GetRotation(), GetTranslation()
    float Ow[3];             // GetCameraCenter()
    float mbf;
    const float* u_right;    // [K.n] mvuRight
    const uint8_t* skip;     // [P.n] isBad() || IsInKeyFrame(pKF) at launch
    int32_t* best_idx;       // [P.n] bestIdx when bestDist <= TH_LOW, else -1
};

// the projection of one point: ProjRec and the right coordinate
struct FuseKfRec {
    float u, v, ur, r;
    int cells;  // the window word of rsc_projcore.h, -1: the point is skipped
};

// :698-738 and the cell range of KeyFrame::GetFeaturesInArea (KeyFrame.cpp:565-579)
RSCM_HD FuseKfRec fkf_setup(const FuseKfProblem& Q, int i, float th) {
    const DevKfpKF& K = Q.K;
    const DevKfpPoints& P = Q.P;
    FuseKfRec q;
    q.u = q.v = q.ur = q.r = 0.0f;
    q.cells = -1;
    const float pw[3] = {P.pos[3 * i], P.pos[3 * i + 1], P.pos[3 * i + 2]};
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        pc[r] = Q.Rcw[3 * r] * pw[0] + Q.Rcw[3 * r + 1] * pw[1] + Q.Rcw[3 * r + 2] * pw[2] + Q.tcw[r];  // :699
    if (pc[2] < 0.0f) return q;      // :702
    const float invz = 1.0f / pc[2];  // :705, a float division
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = K.fx * x + K.cx;  // :709
    const float v = K.fy * y + K.cy;
    if (!(u >= K.min_x && u < K.max_x && v >= K.min_y && v < K.max_y)) return q;  // :713, false for inf / NaN
    const float ur = u - Q.mbf * invz;  // :716
    const float po[3] = {pw[0] - Q.Ow[0], pw[1] - Q.Ow[1], pw[2] - Q.Ow[2]};  // :720
    const float dist = sqrtf((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]);
    const float maxDistance = 1.2f * P.dmax[i];
    const float minDistance = 0.8f * P.dmin[i];
    if (dist < minDistance || dist > maxDistance) return q;  // :724
    const float dot = (po[0] * P.normal[3 * i] + po[1] * P.normal[3 * i + 1]) + po[2] * P.normal[3 * i + 2];
    if ((double)dot < 0.5 * (double)dist) return q;  // :730
    // MapPoint::PredictScale(dist3D, pKF) (MapPoint.cpp:367-382)
    const float ratio = P.dmax[i] / dist;
    int level = (int)ceilf(dm::logf(ratio) / K.log_sf);
    if (level < 0) level = 0;
    else if (level >= K.n_levels) level = K.n_levels - 1;
    const float r = th * K.scale[level];  // :736
    q.cells = proj_cells(K, u, v, r, level);
    q.u = u;
    q.v = v;
    q.ur = ur;
    q.r = r;
    return q;
}

// Everything between GetFeaturesInArea's cell lists and the descriptor distance for keypoint f: the strict
// window (KeyFrame.cpp:589-593), the level (:757) and the reprojection error of the keypoint's kind (:760-784).
// The gate holds the arrays, not the problem (see ProjGate).
struct FuseKfGate {
    const int32_t* octave;
    const ProjPt* kp;
    const float* u_right;
    const float* scale;
    float u, v, ur, r;
    int lo, hi;
    RSCM_HD FuseKfGate(const FuseKfProblem& Q, const FuseKfRec& q)
        : octave(Q.K.octave), kp(Q.K.kp), u_right(Q.u_right), scale(Q.K.scale), u(q.u), v(q.v), ur(q.ur), r(q.r) {
        const int level = ProjCells(q.cells).level;
        lo = level > 0 ? level - 1 : 0;  // octaves are >= 0: [L-1, L] and [max(L-1, 0), L] hold the same keypoints
        hi = level;
    }
    RSCM_HD bool operator()(int f) const {
        const int oct = octave[f];
        if (oct < lo || oct > hi) return false;
        const ProjPt p = kp[f];
        const float ex = u - p.x, ey = v - p.y;
        if (!(fabsf(p.x - u) < r && fabsf(p.y - v) < r)) return false;
        const float sf = scale[oct];
        const float inv_sigma2 = 1.0f / (sf * sf);  // mvInvLevelSigma2[kpLevel]
        const float kpr = u_right[f];
        if (kpr >= 0) {  // :760
            const float er = ur - kpr;
            const float e2 = (ex * ex + ey * ey) + er * er;
            return !((double)(e2 * inv_sigma2) > kFkfChi2Stereo);
        }
        const float e2 = ex * ex + ey * ey;
        return !((double)(e2 * inv_sigma2) > kFkfChi2Mono);
    }
};

// One (point, KeyFrame) pair by one lane: bestIdx when bestDist <= TH_LOW, else -1 (:690-798)
RSCM_HD int fkf_point(const FuseKfProblem& Q, int i, float th) {
    if (!kfp_eligible(Q.P, Q.skip, i)) return -1;  // :695
    const FuseKfRec q = fkf_setup(Q, i, th);
    if (q.cells < 0) return -1;
    return proj_first_min(Q.K, q.cells, Q.P.desc[i], i, KfpAllFree(), FuseKfGate(Q, q), kKfpThLow);
}

#if defined(__HIPCC__)
// grid (pairs, problems); max_points: the largest P.n of the launch
hipError_t launch_fuse_kf(int count, int max_points, const FuseKfProblem* problems, float th, hipStream_t st);
#endif

}  // namespace rsc
