// rsc_localproj.h — Tracking::SearchLocalPoints (src/Tracking.cpp:979-1029) over a flat MapPoint list
// (rsc_mpview) and a resident Frame (rsc_frameview):
//   Frame::isInFrustum(pMP, viewingCosLimit)                            (src/Frame.cpp:336-392)
//   ORBmatcher::SearchByProjection(Frame&, vector<MapPoint>&, th)       (src/ORBmatcher.cpp:16-100)
//   ORBmatcher::RadiusByViewingCos                                      (src/ORBmatcher.cpp:102-108)
// with Frame::GetFeaturesInArea (src/Frame.cpp:394-447): device layout and the per-point arithmetic, shared
// by localproj.hip and the host emulation (tests/localproj_emu).
//
// The matcher is sequentially greedy like the two of rsc_frameproj.h / rsc_kfproj.h, with two differences
// that change the map the rounds iterate:
//
//  1. Occupancy depends on the occupant (:58-60): feature f is skipped only when F.mvpMapPoints[f] is set
//     AND that MapPoint has Observations() > 0.  A point without observations that takes f does not block
//     the points after it: a later point may take f again and overwrite it, and both count in nmatches
//     (the second owner rule of rsc_projcore.h).  An entry occupant with observations (frame_occ == 2)
//     carries kProjOccupied; one without (frame_occ == 1) is free and is overwritten.  The MapPoint left in
//     mvpMapPoints[f] is the LAST claimer (atomicMax over all claims).
//  2. The decision is "best two free candidates, cutoff, ratio veto" (:73-92), not "first free minimum".
//     An earlier point that takes i's best promotes the runner-up; one that takes i's RUNNER-UP can turn a
//     vetoed match into an accepted one.
//
// Mapping, visiting order and the fixed-point argument: rsc_projcore.h, with the owner rule "only claimers
// with observations block" and A[i] = lp_decide(best two of point i's candidates f with owner[f] >= i).
//
// Candidate cache: the four smallest (distance, visiting order) candidates that pass the static gates
// (window, levels, stereo, no entry occupant with observations) and have distance <= keep_max.  Unlike
// rsc_kfproj.h the cutoff TH_HIGH alone is not a sound filter: a runner-up above 100 still vetoes a best
// <= 100 while bestDist > mfNNratio * bestDist2.  lp_veto_bound gives the largest runner-up distance for
// which that can happen for any best <= TH_HIGH under the float expression (124 for 0.8f: 0.8f * 125
// rounds to 100.0f); keep_max = max(TH_HIGH, that bound).  A candidate above keep_max can neither be an
// accepted best nor veto one, and every kept candidate sorts before every dropped one, so dropping them
// leaves every decision unchanged.  When fewer than two cached candidates are free and the list was longer
// than four, the point walks its window again: lp_best here, and on the device the same walk by 16 lanes
// (lp_best_coop in localproj.hip: two smallest (distance, visiting rank) keys instead of the streaming
// update, equal by the equivalence proved in tests/test_cpu_localproj.py).  The finish leaves the LAST
// claimer in out[f] and counts every claim.
//
// Precondition, as in rsc_frameproj.h: an eligible point whose u or v is NaN (camera z == 0 with x == 0 or
// y == 0; the reference feeds NaN to floor there) is outside the reference's defined behaviour and is
// skipped.  z == 0 with x != 0 gives +-inf and is rejected by the image bounds.
#pragma once
#include "rsc_kfproj.h"

namespace rsc {

constexpr int kLpThHigh = 100;  // ORBmatcher::TH_HIGH (ORBmatcher.cpp:8)
constexpr int kLpThreads = 512;
constexpr int kLpMaxFeatures = kProjMaxFeatures;  // Frame::N bound (the LDS owner table)

// what isInFrustum leaves in the MapPoint (Frame.cpp:384-389): mbTrackInView, mTrackProjX, mTrackProjY,
// mTrackProjXR, mnTrackScaleLevel, mTrackViewCos
struct alignas(8) LpTrack {
    int32_t in_view;
    float proj_x, proj_y, proj_xr;
    int32_t level;
    float view_cos;
};

// cached window of one point: what GetFeaturesInArea walks and what the stereo gate compares
struct alignas(16) LpRec {
    float u, v, r, xr;  // mTrackProjX, mTrackProjY, r * mvScaleFactors[level], mTrackProjXR
    int32_t cells;      // as ProjRec::cells
    int32_t in_view;    // the point reaches the matcher's window (counted in nToMatch)
    int32_t pad[2];
};

struct LocalProjProblem {
    const DevProjFrame* F;
    const float* u_right;      // [F.n] mvuRight
    float mbf;
    DevKfpPoints P;
    float Tcw[16];             // mTcw, row-major (fused mode)
    const uint8_t* skip;       // [P.n] mnLastFrameSeen == mCurrentFrame.mnId (Tracking.cpp:1006)
    const uint8_t* has_obs;    // [P.n] Observations() > 0
    const uint8_t* frame_occ;  // [F.n] 0 NULL, 1 set without observations, 2 set with observations
    LpTrack* track;            // [P.n] out (fused mode) / in (matcher-only mode)
    LpRec* rec;                // [P.n] scratch
    ProjCand* cand;            // [P.n] scratch
    int32_t* claim;            // [P.n] scratch: A[i]
    int32_t* out;              // [F.n] index into the points of the MapPoint left in mvpMapPoints[f], else -1
    int32_t* counts;           // [3] nmatches, nToMatch, rounds
};

// ORBmatcher.cpp:102-108: `viewCos>0.998` compares the float with a DOUBLE literal; (float)0.998 is above
// the double 0.998, so a float compare would answer 4.0 there
RSCM_HD float lp_radius(float view_cos) { return (double)view_cos > 0.998 ? 2.5f : 4.0f; }

RSCM_HD LpTrack lp_not_in_view() {
    LpTrack t;
    t.in_view = 0;
    t.proj_x = t.proj_y = t.proj_xr = 0.0f;
    t.level = 0;
    t.view_cos = 0.0f;
    return t;
}

// Tracking.cpp:1006-1009
RSCM_HD bool lp_eligible(const DevKfpPoints& P, const uint8_t* skip, int i) { return P.state[i] == 1 && !skip[i]; }

// Frame::isInFrustum (Frame.cpp:336-392); T = mTcw row-major
RSCM_HD LpTrack lp_frustum(const DevProjFrame& F, float mbf, const DevKfpPoints& P, const float* T, int i,
                           float cos_limit) {
    const LpTrack no = lp_not_in_view();  // :338
    const float pw[3] = {P.pos[3 * i], P.pos[3 * i + 1], P.pos[3 * i + 2]};
    float pc[3], Ow[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pc[r] = T[4 * r] * pw[0] + T[4 * r + 1] * pw[1] + T[4 * r + 2] * pw[2] + T[4 * r + 3];  // :344 mRcw*P+mtcw
        Ow[r] = -(T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]);                            // mOw = -Rcw^T*tcw
    }
    if (pc[2] < 0.0f) return no;                  // :350
    const float invz = 1.0f / pc[2];              // :354, a float division
    const float u = F.fx * pc[0] * invz + F.cx;   // :355 (fx*PcX)*invz
    const float v = F.fy * pc[1] * invz + F.cy;
    if (!(u == u) || !(v == v)) return no;        // NaN: outside the reference's defined behaviour
    if (u < F.min_x || u > F.max_x) return no;    // :358 inclusive bounds
    if (v < F.min_y || v > F.max_y) return no;    // :360
    const float maxDistance = 1.2f * P.dmax[i];   // :364 GetMaxDistanceInvariance
    const float minDistance = 0.8f * P.dmin[i];   // :365
    const float po[3] = {pw[0] - Ow[0], pw[1] - Ow[1], pw[2] - Ow[2]};                          // :366
    const float dist = sqrtf((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]);                  // :367
    if (dist < minDistance || dist > maxDistance) return no;                                    // :369
    const float dot = (po[0] * P.normal[3 * i] + po[1] * P.normal[3 * i + 1]) + po[2] * P.normal[3 * i + 2];
    const float viewCos = dot / dist;             // :375, a float division
    if (viewCos < cos_limit) return no;           // :377, compared in float
    // :381 MapPoint::PredictScale(dist, Frame*) (MapPoint.cpp:384-398), as proj_setup
    const float ratio = P.dmax[i] / dist;
    int level = (int)ceilf(dm::logf(ratio) / F.log_sf);
    if (level < 0) level = 0;
    else if (level >= F.n_levels) level = F.n_levels - 1;
    LpTrack t;
    t.in_view = 1;                 // :384
    t.proj_x = u;                  // :385
    t.proj_xr = u - mbf * invz;    // :386
    t.proj_y = v;                  // :387
    t.level = level;               // :388
    t.view_cos = viewCos;          // :389
    return t;
}

RSCM_HD LpRec lp_no_window() {
    LpRec q;
    q.u = q.v = q.r = q.xr = 0.0f;
    q.cells = -1;
    q.in_view = 0;
    q.pad[0] = q.pad[1] = 0;
    return q;
}

// ORBmatcher.cpp:31-40 and the cell range of GetFeaturesInArea (Frame.cpp:399-413).  The level of `t` must
// be in [0, F.n_levels).
RSCM_HD LpRec lp_window(const DevProjFrame& F, const LpTrack& t, float th) {
    LpRec q = lp_no_window();
    if (!t.in_view) return q;                          // :25
    const float u = t.proj_x, v = t.proj_y;
    if (!(u == u) || !(v == v)) return q;              // the precondition above
    q.in_view = 1;
    float r = lp_radius(t.view_cos);                   // :34
    if (th != 1.0f) r *= th;                           // :20, :36-37
    const float rad = r * F.scale[t.level];            // :40
    q.u = u;
    q.v = v;
    q.r = rad;
    q.xr = t.proj_xr;
    q.cells = proj_cells(F, u, v, rad, t.level);
    return q;
}

// the static gates of point q: levels [L-1, L], the window, then the stereo gate (ORBmatcher.cpp:62-67)
RSCM_HD ProjStereoGate lp_gate(const DevProjFrame& F, const float* u_right, const LpRec& q) {
    const int level = ProjCells(q.cells).level;
    return ProjStereoGate{ProjGate(F, q.u, q.v, q.r, level - 1, level), u_right, q.xr};
}

// :47-51 and the streaming update of :73-85: equal to "the two smallest under (distance, visiting order)"
struct LpTop2 {
    int bestDist, bestLevel, bestDist2, bestLevel2, bestIdx;
};
RSCM_HD LpTop2 lp_top2_init() {
    LpTop2 t;
    t.bestDist = 256;
    t.bestLevel = -1;
    t.bestDist2 = 256;
    t.bestLevel2 = -1;
    t.bestIdx = -1;
    return t;
}
RSCM_HD void lp_top2_push(LpTop2& t, int dist, int level, int idx) {
    if (dist < t.bestDist) {          // :73
        t.bestDist2 = t.bestDist;
        t.bestDist = dist;
        t.bestLevel2 = t.bestLevel;
        t.bestLevel = level;
        t.bestIdx = idx;
    } else if (dist < t.bestDist2) {  // :81
        t.bestLevel2 = level;
        t.bestDist2 = dist;
    }
}
// :89-95: the feature the point takes, or -1.  The veto compares an int with a FLOAT product.
RSCM_HD int lp_decide(const LpTop2& t, float nn_ratio) {
    if (t.bestDist > kLpThHigh) return -1;
    if (t.bestLevel == t.bestLevel2 && (float)t.bestDist > nn_ratio * (float)t.bestDist2) return -1;
    return t.bestIdx;
}

// The largest bestDist2 in [0, 256] that vetoes some bestDist <= TH_HIGH (bestDist = TH_HIGH is the easiest
// to veto), -1 when none does.  nn_ratio >= 0: the product is monotone in bestDist2, so every larger value
// vetoes nothing either.
RSCM_HD int lp_veto_bound(float nn_ratio) {
    int b = -1;
    for (int d2 = 0; d2 <= 256; ++d2)
        if ((float)kLpThHigh > nn_ratio * (float)d2) b = d2;
    return b;
}
RSCM_HD int lp_keep_max(float nn_ratio) {
    const int b = lp_veto_bound(nn_ratio);
    return b > kLpThHigh ? b : kLpThHigh;
}

// :54-95 over the window of `q`: the feature point i takes when the features with owner[f] < i are skipped
// (an entry occupant with observations carries kProjOccupied), or -1
template <class OwnerPtr>
RSCM_HD int lp_best(const DevProjFrame& F, const float* u_right, const LpRec q, const ProjDesc dMP, int i,
                    OwnerPtr owner, float nn_ratio) {
    if (q.cells < 0) return -1;
    const ProjStereoGate gate = lp_gate(F, u_right, q);
    const ProjDesc* desc = F.desc;
    LpTop2 t = lp_top2_init();
    proj_walk(F, ProjCells(q.cells), [&](int f) {
        if (!gate(f) || owner[f] < i) return;  // :58-60
        lp_top2_push(t, proj_desc_dist(dMP, desc[f]), gate.g.octave[f], f);
    });
    return lp_decide(t, nn_ratio);
}

// One round's choice from the cached candidates: the feature, -1 for none, or -2 when fewer than two of
// the cached four are free and the list was longer (lp_best then walks the window).  The cache is a prefix
// of the candidates sorted by (distance, visiting order), so its first two free entries are the best and
// the runner-up of the walk.
template <class OwnerPtr>
RSCM_HD int lp_pick(const DevProjFrame& F, const ProjCand cd, bool more, int i, OwnerPtr owner, float nn_ratio) {
    LpTop2 t = lp_top2_init();
    int found = 0;
    bool complete = !more;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (found == 2) break;
        const int c = cd.c[k];
        if (c < 0) {
            complete = true;
            break;
        }
        const int f = c & 0xffff;
        if (owner[f] < i) continue;
        lp_top2_push(t, c >> 16, F.octave[f], f);
        ++found;
    }
    if (found < 2 && !complete) return -2;
    return lp_decide(t, nn_ratio);
}

// the cache of point q: distance <= keep_max on features without an entry occupant that has observations; true
// when more than four qualified
RSCM_HD bool lp_candidates(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP,
                           const uint8_t* frame_occ, int keep_max, ProjCand& out) {
    return proj_candidates(F, q.cells, dMP, lp_gate(F, u_right, q), [frame_occ](int f) { return frame_occ[f] == 2; },
                           keep_max, out);
}

// What the rounds share, for point i: isInFrustum (fused: its record goes to the caller-visible `track`; else
// the caller's record is read from there), the window, the cache and an empty claim
RSCM_HD void lp_setup_point(const LocalProjProblem& Q, int i, int fused, float cos_limit, float th, int keep_max) {
    const DevProjFrame& F = *Q.F;
    LpTrack t = lp_not_in_view();
    const bool eligible = lp_eligible(Q.P, Q.skip, i);
    if (fused) {
        if (eligible) t = lp_frustum(F, Q.mbf, Q.P, Q.Tcw, i, cos_limit);
        Q.track[i] = t;
    } else if (eligible) {
        t = Q.track[i];
        if ((unsigned)t.level >= (unsigned)F.n_levels) t.in_view = 0;  // the host checked it; never index past scale[]
    }
    LpRec q = lp_window(F, t, th);
    ProjCand cd = proj_no_cand();
    if (q.cells >= 0 && lp_candidates(F, Q.u_right, q, Q.P.desc[i], Q.frame_occ, keep_max, cd)) q.cells |= kProjMore;
    Q.rec[i] = q;
    Q.cand[i] = cd;
    Q.claim[i] = -1;
}

// the matcher of the rounds (rsc_projrounds.h); localproj.hip adds best_coop
struct LpRounds {
    static constexpr bool kCoopWalk = true;
    const LocalProjProblem& Q;
    float nn_ratio;
    RSCM_HD int n_points() const { return Q.P.n; }
    RSCM_HD bool entry_occupied(int f) const { return Q.frame_occ[f] == 2; }
    RSCM_HD bool blocks(int i) const { return Q.has_obs[i] != 0; }  // a point without observations blocks nobody
    RSCM_HD int pick(int i, const int* owner) const {
        const int cells = Q.rec[i].cells;
        return cells < 0 ? kProjSkip : lp_pick(*Q.F, Q.cand[i], (cells & kProjMore) != 0, i, owner, nn_ratio);
    }
    RSCM_HD int best(int i, const int* owner) const {
        return lp_best(*Q.F, Q.u_right, Q.rec[i], Q.P.desc[i], i, owner, nn_ratio);
    }
};

#if defined(__HIPCC__)
// fused != 0: the setup kernel runs isInFrustum and writes `track`; else it reads `track`.  mid (may be
// NULL): recorded between the setup kernel and the rounds kernel.
hipError_t launch_search_local_points(int count, int max_points, const LocalProjProblem* problems, int fused,
                                      float cos_limit, float th, float nn_ratio, hipEvent_t mid, hipStream_t st);
#endif

}  // namespace rsc
