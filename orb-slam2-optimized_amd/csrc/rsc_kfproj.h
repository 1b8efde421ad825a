// rsc_kfproj.h — the loop-closing projection matchers over a flat MapPoint list (rsc_mpview):
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)   (src/ORBmatcher.cpp:241-352)
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)            (src/ORBmatcher.cpp:823-946)
// with KeyFrame::GetFeaturesInArea / IsInImage (src/KeyFrame.cpp:560-604): device layout and the per-point
// arithmetic, shared by kfproj.hip and the host emulation (tests/kfproj_emu).
//
// SearchByProjection is sequentially greedy: point i skips the keypoints that earlier points of the call
// wrote to vpMatched (:324).  Mapping, visiting order, candidate cache and the fixed-point argument:
// rsc_projcore.h, with the points in the point role and the KeyFrame's keypoints in the feature role.  What
// this matcher sets: every claimer blocks; a keypoint with vpMatched[f] != NULL on entry is occupied; levels
// [L-1, L]; the decision is "first free minimum, kept if <= TH_LOW"; the finish keeps owner[A[i]] == i.
// Keeping only candidates with distance <= TH_LOW in the cache is sound: a point takes its minimum over the
// free keypoints first and applies the cutoff afterwards, so a candidate above the cutoff can only ever produce
// "no match", which is what an exhausted list produces too.
// Fuse has no such coupling (it never skips a keypoint): one lane per (point, KeyFrame) pair.
//
// What differs from the Frame matcher (rsc_frameproj.h), line by line below: z < 0 is rejected; invz is a
// float division in SearchByProjection (:280) and a double division rounded to float in Fuse (:865); u =
// fx*(x*invz)+cx; the image bounds exclude the maximum; the viewing-angle test PO.Pn < 0.5*dist compares
// a float dot product (summed left to right, as every fixed-size sum here) with a double product, in
// double; levels [L-1, L]; cutoff TH_LOW = 50; no orientation check.  z == 0 is defined behaviour here:
// invz is +-inf, u / v are inf or NaN, IsInImage is false and the point is skipped.
//
// Scw quirk, kept: Converter::toIso(g2o::Sim3) (src/Converter.cpp:31-37) stores the UNIT rotation in
// linear() and the translation of the Sim3 (not divided by s) in translation(), and SearchByProjection
// uses them as they are: Ow = -R^T t with no division by the scale.  Fuse receives s*R and normalises:
// scw = sqrt(row0.row0), Rcw = sRcw / scw, tcw = t / scw (:832-836).
//
// Precondition of both calls: the points of a view are distinct MapPoints (LoopClosing.cpp:350-353
// guarantees it through mnLoopPointForKF); a duplicate would be a second point the `already` /
// vpMatched bookkeeping of the reference treats as the same object.
#pragma once
#include "rsc_frameproj.h"

namespace rsc {

constexpr int kKfpThLow = 50;          // ORBmatcher::TH_LOW (ORBmatcher.cpp:7)
constexpr int kKfpMaxKeypoints = kProjMaxFeatures;  // KeyFrame::N bound (the LDS owner table)
constexpr int kKfpThreads = 512;

// The KeyFrame as the two matchers read it (the keypoint side of rsc_kfview): the Frame view with angle == NULL
// (no rotation check).  A type of its own only for the constructor, which takes the fields without the angle.
struct DevKfpKF : DevProjFrame {
    DevKfpKF() = default;
    RSCM_HD DevKfpKF(const ProjPt* kp, const int32_t* octave, const ProjDesc* desc, const int32_t* cell_begin,
                     const int32_t* cell_feat, const float* scale, float min_x, float max_x, float min_y, float max_y,
                     float gw_inv, float gh_inv, float fx, float fy, float cx, float cy, float log_sf, int n,
                     int n_levels)
        : DevProjFrame{kp, octave, nullptr, desc, cell_begin, cell_feat, scale, min_x, max_x, min_y, max_y,
                       gw_inv, gh_inv, fx, fy, cx, cy, log_sf, n, n_levels} {}
};

// vpPoints (rsc_mpview)
struct DevKfpPoints {
    const uint8_t* state;  // [n] 1 good, 2 isBad()
    const float* pos;      // [n][3] GetWorldPos()
    const float* normal;   // [n][3] GetNormal()
    const float* dmax;     // [n] mfMaxDistance
    const float* dmin;     // [n] mfMinDistance
    const ProjDesc* desc;  // [n] GetDescriptor()
    int n;
};

struct KfProjProblem {
    DevKfpKF K;
    DevKfpPoints P;
    float Scw[16];            // mScw, row-major
    const uint8_t* already;   // [P.n] spAlreadyFound.count(pMP)
    const uint8_t* occupied;  // [K.n] vpMatched[idx] != NULL on entry
    ProjRec* rec;             // [P.n] scratch
    ProjCand* cand;           // [P.n] scratch
    int32_t* claim;           // [P.n] scratch: A[i]
    int32_t* out;             // [K.n] index into the points of the MapPoint written to vpMatched[idx], else -1
    int32_t* nmatches;        // [1]
    int32_t* rounds;          // [1]
};

struct KfFuseProblem {
    DevKfpKF K;
    float Scw[16];           // Scw with linear() = s * R, row-major
    const uint8_t* in_kf;    // [points n] pKF->GetMapPoints().count(pMP)
    int32_t* best_idx;       // [points n] bestIdx when bestDist <= TH_LOW, else -1
};

// an owner table in which every keypoint is free (Fuse)
struct KfpAllFree {
    RSCM_HD int operator[](int) const { return kProjFree; }
};

// :266 / :851
RSCM_HD bool kfp_eligible(const DevKfpPoints& P, const uint8_t* skip, int i) { return P.state[i] == 1 && !skip[i]; }

// :270-309 (fuse = false) or :855-895 (fuse = true) and the cell range of KeyFrame::GetFeaturesInArea
// (KeyFrame.cpp:565-579).  R, t: what the caller decomposed Scw into (kfp_decompose).
RSCM_HD ProjRec kfp_setup(const DevKfpKF& K, const DevKfpPoints& P, const float* R, const float* t, int i, float th,
                          bool fuse) {
    const ProjRec q = proj_no_window();
    const float pw[3] = {P.pos[3 * i], P.pos[3 * i + 1], P.pos[3 * i + 2]};
    float pc[3], Ow[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pc[r] = R[3 * r] * pw[0] + R[3 * r + 1] * pw[1] + R[3 * r + 2] * pw[2] + t[r];  // Rcw*p3Dw+tcw
        Ow[r] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);                     // -Rcw^T*tcw
    }
    if (pc[2] < 0.0f) return q;  // :276 compares with the double 0.0, :861 with 0.0f: the same set of floats
    // :280 `1/p3Dc.z()` is a float division, :865 `1.0/p3Dc.z()` a double one rounded to float
    const float invz = fuse ? (float)(1.0 / (double)pc[2]) : 1.0f / pc[2];
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = K.fx * x + K.cx;  // fx*(xc*invz), the SearchBySim3 grouping
    const float v = K.fy * y + K.cy;
    // KeyFrame::IsInImage: x >= min && x < max (false for the inf / NaN of z == 0)
    if (!(u >= K.min_x && u < K.max_x && v >= K.min_y && v < K.max_y)) return q;
    const float po[3] = {pw[0] - Ow[0], pw[1] - Ow[1], pw[2] - Ow[2]};
    const float dist = sqrtf((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]);
    const float maxDistance = 1.2f * P.dmax[i];  // GetMaxDistanceInvariance
    const float minDistance = 0.8f * P.dmin[i];
    if (dist < minDistance || dist > maxDistance) return q;
    // :303 `PO.dot(Pn) < 0.5*dist`: float dot product against a double product
    const float dot = (po[0] * P.normal[3 * i] + po[1] * P.normal[3 * i + 1]) + po[2] * P.normal[3 * i + 2];
    if ((double)dot < 0.5 * (double)dist) return q;
    // MapPoint::PredictScale(dist, pKF) (MapPoint.cpp:367-382)
    const float ratio = P.dmax[i] / dist;
    int level = (int)ceilf(dm::logf(ratio) / K.log_sf);
    if (level < 0) level = 0;
    else if (level >= K.n_levels) level = K.n_levels - 1;
    const float r = th * K.scale[level];
    ProjRec w;
    w.u = u;
    w.v = v;
    w.r = r;
    w.cells = proj_cells(K, u, v, r, level);
    return w.cells < 0 ? q : w;
}

// SearchByProjection uses Scw as toIso left it (:250-251); Fuse divides by the scale (:832-835).
RSCM_HD void kfp_decompose(const float* S, bool fuse, float* R, float* t) {
    float scw = 1.0f;
    if (fuse) scw = sqrtf((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = fuse ? S[4 * r + c] / scw : S[4 * r + c];
        t[r] = fuse ? S[4 * r + 3] / scw : S[4 * r + 3];
    }
}

// the static gates of point q: the window (KeyFrame.cpp:589-593) and levels [L-1, L] (:329 / :913)
RSCM_HD ProjGate kfp_gate(const DevKfpKF& K, const ProjRec& q) {
    const int level = ProjCells(q.cells).level;
    return ProjGate(K, q.u, q.v, q.r, level - 1, level);
}

// :319-343 / :906-928 over the window of `q`: the keypoint point i takes when the keypoints with owner[f] < i
// are not available, or -1.  bestDist starts at 256 (:319) or INT_MAX (:906); with the cutoff at TH_LOW the two
// give the same answer.
template <class OwnerPtr>
RSCM_HD int kfp_best(const DevKfpKF& K, const ProjRec& q, const ProjDesc& dMP, int i, OwnerPtr owner) {
    return proj_first_min(K, q.cells, dMP, i, owner, kfp_gate(K, q), kKfpThLow);
}

// the cache of point q: distance <= TH_LOW on keypoints free before the call; true when more than four qualified
RSCM_HD bool kfp_candidates(const DevKfpKF& K, const ProjRec& q, const ProjDesc& dMP, const uint8_t* occupied,
                            ProjCand& out) {
    return proj_candidates(K, q.cells, dMP, kfp_gate(K, q), [occupied](int f) { return occupied[f] != 0; },
                           kKfpThLow, out);
}

// What the rounds share, for point i: the window, the cache and an empty claim
RSCM_HD void kfp_setup_point(const KfProjProblem& Q, int i, float th) {
    ProjRec q = proj_no_window();
    ProjCand cd = proj_no_cand();
    if (kfp_eligible(Q.P, Q.already, i)) {
        float R[9], t[3];
        kfp_decompose(Q.Scw, false, R, t);
        q = kfp_setup(Q.K, Q.P, R, t, i, th, false);
        if (q.cells >= 0 && kfp_candidates(Q.K, q, Q.P.desc[i], Q.occupied, cd)) q.cells |= kProjMore;
    }
    Q.rec[i] = q;
    Q.cand[i] = cd;
    Q.claim[i] = -1;
}

// the matcher of the rounds (rsc_projrounds.h)
struct KfpRounds {
    static constexpr bool kCoopWalk = false;
    const KfProjProblem& Q;
    RSCM_HD int n_points() const { return Q.P.n; }
    RSCM_HD bool entry_occupied(int f) const { return Q.occupied[f] != 0; }
    RSCM_HD bool blocks(int) const { return true; }  // :324
    RSCM_HD int pick(int i, const int* owner) const {
        const int cells = Q.rec[i].cells;
        return cells < 0 ? kProjSkip : proj_pick(Q.cand[i], (cells & kProjMore) != 0, i, owner);
    }
    RSCM_HD int best(int i, const int* owner) const {  // :319-343
        return kfp_best(Q.K, Q.rec[i], Q.P.desc[i], i, owner);
    }
};

// Fuse for one (point, KeyFrame) pair: bestIdx when bestDist <= TH_LOW, else -1 (:846-928)
RSCM_HD int kfp_fuse_point(const DevKfpKF& K, const DevKfpPoints& P, const float* Scw, const uint8_t* in_kf, int i,
                           float th) {
    if (!kfp_eligible(P, in_kf, i)) return -1;
    float R[9], t[3];
    kfp_decompose(Scw, true, R, t);
    const ProjRec q = kfp_setup(K, P, R, t, i, th, true);
    if (q.cells < 0) return -1;
    return kfp_best(K, q, P.desc[i], i, KfpAllFree());
}

#if defined(__HIPCC__)
hipError_t launch_search_by_projection_kf(int count, int max_points, const KfProjProblem* problems, float th,
                                          hipStream_t st);
hipError_t launch_fuse_sim3(int count, const DevKfpPoints* points, int n_points, const KfFuseProblem* problems,
                            float th, hipStream_t st);
#endif

}  // namespace rsc
