// rsc_frameproj.h — ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist)
// (src/ORBmatcher.cpp:1317-1444 with Frame::GetFeaturesInArea, src/Frame.cpp:394-447): device layout
// and the per-MapPoint arithmetic, shared by frameproj.hip and the host emulation (tests/frameproj_emu).
//
// The matcher is sequentially greedy: MapPoint i skips the Frame features that earlier MapPoints
// claimed (:1386-1387).  Mapping, visiting order, candidate cache and the fixed-point argument: rsc_projcore.h.
// What this matcher sets: every claimer blocks; a feature with frame_mp[f] >= 0 is occupied on entry; levels
// [L-1, L+1]; the decision is "first free minimum, kept if <= ORBdist"; the finish keeps owner[A[i]] == i and
// runs the rotation check on those.
//
// Float conventions are those of oracle/sim3match_oracle.h (rows summed left to right, invz through a
// double division, logf as the float rounding of dm::log); what differs from SearchBySim3 is stated
// at each line.  Precondition: no eligible MapPoint has camera z == 0 (the reference feeds NaN to
// floor there); such a point is skipped.
#pragma once
#include "rsc_projcore.h"

namespace rsc {

constexpr int kProjThreads = 512;

// the candidate KeyFrame's MapPoints
struct DevProjKF {
    const uint8_t* mp_state;  // [n] 0 NULL, 1 good, 2 isBad()
    const float* mp_pos;      // [n][3]
    const float* mp_dmax;     // [n] mfMaxDistance
    const float* mp_dmin;     // [n] mfMinDistance
    const ProjDesc* mp_desc;  // [n]
    const float* angle;       // [n] mvKeysUn[i].angle, NULL without rsc_kfview_set_angles
    int n;
};

// cached projection of one MapPoint: the window GetFeaturesInArea walks
struct alignas(16) ProjRec {
    float u, v, r;
    int32_t cells;  // -1: no window; else minX | maxX << 6 | minY << 12 | maxY << 18 | level << 24 | kProjMore
};

struct FrameProjProblem {
    const DevProjFrame* F;
    DevProjKF K;
    float Tcw[16];            // CurrentFrame.mTcw, row-major
    const uint8_t* already;   // [K.n] sAlreadyFound.count(vpMPs[i])
    const int32_t* frame_mp;  // [F.n] >= 0: CurrentFrame.mvpMapPoints[f] is set
    ProjRec* rec;             // [K.n] scratch
    ProjCand* cand;           // [K.n] scratch
    int32_t* claim;           // [K.n] scratch: A[i]
    int32_t* out;             // [F.n] KeyFrame slot of each surviving new match, else -1
    int32_t* nmatches;        // [1]
    int32_t* rounds;          // [1]
};

// :1337-1339
RSCM_HD bool proj_eligible(const DevProjKF& K, const uint8_t* already, int i) {
    return K.mp_state[i] == 1 && !already[i];
}

// :1341-1373 and the cell range of GetFeaturesInArea (Frame.cpp:399-413)
RSCM_HD ProjRec proj_no_window() {
    ProjRec q;
    q.u = q.v = q.r = 0.0f;
    q.cells = -1;
    return q;
}

RSCM_HD ProjRec proj_setup(const DevProjFrame& F, const DevProjKF& K, const float* T, int i, float th) {
    const ProjRec q = proj_no_window();
    const float pw[3] = {K.mp_pos[3 * i], K.mp_pos[3 * i + 1], K.mp_pos[3 * i + 2]};
    float pc[3], Ow[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pc[r] = T[4 * r] * pw[0] + T[4 * r + 1] * pw[1] + T[4 * r + 2] * pw[2] + T[4 * r + 3];  // Rcw*x3Dw+tcw
        Ow[r] = -(T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]);                            // -Rcw^T*tcw
    }
    const float invzc = (float)(1.0 / (double)pc[2]);  // `const float invzc = 1.0/x3Dc.z()` (:1347)
    const float u = F.fx * pc[0] * invzc + F.cx;       // (fx*xc)*invzc: not SearchBySim3's fx*(xc*invz)
    const float v = F.fy * pc[1] * invzc + F.cy;
    if (!(u == u) || !(v == v)) return q;              // z == 0: outside the reference's defined behaviour
    if (u < F.min_x || u > F.max_x) return q;          // inclusive bounds, and no z > 0 test (:1352-1355)
    if (v < F.min_y || v > F.max_y) return q;
    const float po[3] = {pw[0] - Ow[0], pw[1] - Ow[1], pw[2] - Ow[2]};
    const float dist3D = sqrtf((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]);
    const float maxDistance = 1.2f * K.mp_dmax[i];     // GetMaxDistanceInvariance
    const float minDistance = 0.8f * K.mp_dmin[i];
    if (dist3D < minDistance || dist3D > maxDistance) return q;
    // MapPoint::PredictScale(dist3D, &CurrentFrame) (MapPoint.cpp:384-398)
    const float ratio = K.mp_dmax[i] / dist3D;
    int level = (int)ceilf(dm::logf(ratio) / F.log_sf);
    if (level < 0) level = 0;
    else if (level >= F.n_levels) level = F.n_levels - 1;
    const float r = th * F.scale[level];
    ProjRec w;
    w.u = u;
    w.v = v;
    w.r = r;
    w.cells = proj_cells(F, u, v, r, level);
    return w.cells < 0 ? q : w;
}

// the static gates of MapPoint q: levels [L-1, L+1] (bCheckLevels true) and the window
RSCM_HD ProjGate proj_gate(const DevProjFrame& F, const ProjRec& q) {
    const int level = ProjCells(q.cells).level;
    return ProjGate(F, q.u, q.v, q.r, level - 1, level + 1);
}

// :1380-1400 over the window of `q`: the feature MapPoint i takes when the features with owner[f] < i are not
// available, or -1
template <class OwnerPtr>
RSCM_HD int proj_best(const DevProjFrame& F, const ProjRec& q, const ProjDesc& dMP, int i, OwnerPtr owner,
                      int orb_dist) {
    return proj_first_min(F, q.cells, dMP, i, owner, proj_gate(F, q), orb_dist);
}

// The cache of MapPoint q: distance <= ORBdist on features free before the call; bestDist starts at 256 under a
// strict < (:1380), so 256 and above never match either.  Returns true when more than four qualified.
RSCM_HD bool proj_candidates(const DevProjFrame& F, const ProjRec& q, const ProjDesc& dMP, const int32_t* frame_mp,
                             int orb_dist, ProjCand& out) {
    return proj_candidates(F, q.cells, dMP, proj_gate(F, q), [frame_mp](int f) { return frame_mp[f] >= 0; },
                           orb_dist < 255 ? orb_dist : 255, out);
}

// What the rounds share, for MapPoint i: the window, the cache and an empty claim
RSCM_HD void proj_setup_point(const FrameProjProblem& P, int i, float th, int orb_dist) {
    const DevProjFrame& F = *P.F;
    ProjRec q = proj_no_window();
    ProjCand cd = proj_no_cand();
    if (proj_eligible(P.K, P.already, i)) {
        q = proj_setup(F, P.K, P.Tcw, i, th);
        if (q.cells >= 0 && proj_candidates(F, q, P.K.mp_desc[i], P.frame_mp, orb_dist, cd)) q.cells |= kProjMore;
    }
    P.rec[i] = q;
    P.cand[i] = cd;
    P.claim[i] = -1;
}

// the matcher of the rounds (rsc_projrounds.h); Occ(f): CurrentFrame.mvpMapPoints[f] is set on entry
template <class Occ>
struct FrameRounds {
    static constexpr bool kCoopWalk = false;
    const FrameProjProblem& P;
    int orb_dist;
    Occ occ;
    RSCM_HD int n_points() const { return P.K.n; }
    RSCM_HD bool entry_occupied(int f) const { return occ(f); }
    RSCM_HD bool blocks(int) const { return true; }  // mvpMapPoints[i2] set (:1386): before the call or by j < i
    RSCM_HD int pick(int i, const int* owner) const {
        const int cells = P.rec[i].cells;
        return cells < 0 ? kProjSkip : proj_pick(P.cand[i], (cells & kProjMore) != 0, i, owner);
    }
    RSCM_HD int best(int i, const int* owner) const {  // :1380-1400
        return proj_best(*P.F, P.rec[i], P.K.mp_desc[i], i, owner, orb_dist);
    }
};

#if defined(__HIPCC__)
hipError_t launch_search_by_projection(int count, int max_kf_points, const FrameProjProblem* problems, float th,
                                       int orb_dist, int check_orientation, hipStream_t st);
#endif

}  // namespace rsc
