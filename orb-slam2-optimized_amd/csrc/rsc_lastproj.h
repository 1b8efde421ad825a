// rsc_lastproj.h — ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
// (src/ORBmatcher.cpp:1173-1315, the matcher of Tracking::TrackWithMotionModel, src/Tracking.cpp:732,738) with
// Frame::GetFeaturesInArea (src/Frame.cpp:394-447) over a resident current Frame (rsc_frameview with
// rsc_frameview_set_stereo) and the last Frame's slots (rsc_lastframe): device layout and the per-point
// arithmetic, shared by lastproj.hip and the host emulation (tests/lastproj_emu).
//
// Per LastFrame slot i with a MapPoint that is not an outlier, in slot order:
//   projection   x3Dc = Rcw*x3Dw + tcw, invzc through a double division, invzc < 0 rejects, (fx*xc)*invzc + cx,
//                inclusive image bounds: the arithmetic of rsc_frameproj.h (:1205-1221)
//   radius       th * mvScaleFactors[LastFrame.mvKeys[i].octave]; no PredictScale, no distance test (:1223-1226)
//   levels       one mode per call from tlc.z against mb (:1186-1194, last_mode): forward takes octaves >= o
//                with no upper bound, backward [0, o], else [o-1, o+1] (:1230-1235)
//   candidates   skipped when mvpMapPoints[i2] is set AND has Observations() > 0 (:1248-1250), and by the stereo
//                gate when mvuRight[i2] > 0 (:1252-1258); first strict minimum of the descriptor distance
//   acceptance   bestDist <= TH_HIGH (:1271); every accepted claim is one rotHist entry (:1276-1286)
//
// Occupancy depends on the occupant as in rsc_localproj.h: a slot whose MapPoint has no observations (the
// visual-odometry points of UpdateLastFrame) takes a feature and blocks nobody.  Mapping, visiting order and
// the fixed-point argument: rsc_projcore.h, with the owner rule "only claimers with observations block",
// kProjOccupied for an entry occupant with observations, and the decision "first free minimum, kept if <=
// TH_HIGH" as in rsc_frameproj.h.
//
// Candidate cache: distance <= TH_HIGH.  TH_HIGH IS a sound filter here, unlike in rsc_localproj.h: the point
// takes its minimum over the free features first and applies the cutoff afterwards, and there is no runner-up
// test.  If the free minimum is above TH_HIGH the point claims nothing, and so it does when every free
// candidate was dropped; if it is <= TH_HIGH it was kept.  When all four cached candidates are taken by lower
// slots and there were more, the window is walked again (on the device by 16 lanes).
//
// Rotation check (:1292-1312).  The histogram holds one entry PER CLAIM, overwritten claims included, and
// the removal runs per entry: mvpMapPoints[f] ends up nullptr when ANY claimer of f fell into a removed bin,
// even if the last claimer's bin was kept, and nmatches is (claims) - (claims in removed bins), which can
// differ from the number of slots the call leaves set.
//
// Precondition, as in rsc_frameproj.h: a point whose u or v is NaN (camera z == 0 with x == 0 or y == 0, or a
// non-finite position; the reference feeds NaN to floor there) is outside the reference's defined behaviour
// and is skipped.  z == 0 with x != 0 gives +-inf and is rejected by the image bounds.
#pragma once
#include "rsc_localproj.h"

namespace rsc {

constexpr int kLastThreads = kLpThreads;
constexpr int kLastMaxFeatures = kProjMaxFeatures;  // CurrentFrame.N bound (the LDS owner table)
constexpr int kLastMaxSlots = 8192;                 // LastFrame.N bound
constexpr int kLastWindow = 0, kLastForward = 1, kLastBackward = 2;  // the level mode of a call
constexpr int kLastNulled = -2;                     // out[f]: the rotation check set mvpMapPoints[f] = nullptr

// the last Frame as the matcher reads it
struct DevLastFrame {
    const int32_t* octave;     // [n] mvKeys[i].octave
    const float* angle;        // [n] mvKeysUn[i].angle
    const uint8_t* mp_state;   // [n] 0 NULL, 1 set, 2 set and mvbOutlier[i]
    const float* mp_pos;       // [n][3] GetWorldPos()
    const ProjDesc* mp_desc;   // [n] MapPoint::GetDescriptor()
    const uint8_t* mp_has_obs; // [n] Observations() > 0
    int n;
};

struct LastProjProblem {
    const DevProjFrame* F;
    const float* u_right;      // [F.n] mvuRight
    float mbf;
    int32_t mode;              // last_mode()
    DevLastFrame L;
    float Tcw[16];             // CurrentFrame.mTcw, row-major
    const uint8_t* frame_occ;  // [F.n] 0 NULL, 1 set without observations, 2 set with observations
    LpRec* rec;                // [L.n] scratch
    ProjCand* cand;            // [L.n] scratch
    int32_t* claim;            // [L.n] scratch: A[i]
    int32_t* out;              // [F.n] >= 0 the LastFrame slot left in mvpMapPoints[f], -1 untouched, -2 nulled
    int32_t* counts;           // [4] nmatches, mode, rounds, claims
};

// :1183-1194.  Tc = CurrentFrame.mTcw, Tl = LastFrame.mTcw, row-major; only tlc.z is needed
RSCM_HD int last_mode(const float* Tc, const float* Tl, float mb) {
    float twc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) twc[r] = -(Tc[r] * Tc[3] + Tc[4 + r] * Tc[7] + Tc[8 + r] * Tc[11]);  // -Rcw^T*tcw
    const float tlcz = (Tl[8] * twc[0] + Tl[9] * twc[1] + Tl[10] * twc[2]) + Tl[11];                 // Rlw*twc+tlw
    if (tlcz > mb) return kLastForward;    // :1193, tested first (:1230)
    if (-tlcz > mb) return kLastBackward;  // :1194
    return kLastWindow;
}

// :1230-1235 with the level test of GetFeaturesInArea (Frame.cpp:415,428-435): the octaves [lo, hi] taken.
// Forward: minLevel = o, maxLevel = -1 (no upper bound; o == 0 switches the check off, the same set).
RSCM_HD void last_levels(int mode, int o, int& lo, int& hi) {
    if (mode == kLastForward) {
        lo = o;
        hi = INT_MAX;
    } else if (mode == kLastBackward) {
        lo = 0;
        hi = o;
    } else {
        lo = o - 1;
        hi = o + 1;
    }
}

// :1198-1202
RSCM_HD bool last_eligible(const DevLastFrame& L, int i) { return L.mp_state[i] == 1; }

// :1205-1226 and the cell range of GetFeaturesInArea (Frame.cpp:399-413).  The slot's octave must be in
// [0, F.n_levels).
RSCM_HD LpRec last_setup(const DevProjFrame& F, float mbf, const DevLastFrame& L, const float* T, int i, float th) {
    LpRec q = lp_no_window();
    const float pw[3] = {L.mp_pos[3 * i], L.mp_pos[3 * i + 1], L.mp_pos[3 * i + 2]};
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        pc[r] = T[4 * r] * pw[0] + T[4 * r + 1] * pw[1] + T[4 * r + 2] * pw[2] + T[4 * r + 3];  // :1206
    const float invzc = (float)(1.0 / (double)pc[2]);  // `const float invzc = 1.0/x3Dc.z()` (:1210)
    if (invzc < 0.0f) return q;                        // :1212
    const float u = F.fx * pc[0] * invzc + F.cx;       // :1215 (fx*xc)*invzc
    const float v = F.fy * pc[1] * invzc + F.cy;
    if (!(u == u) || !(v == v)) return q;              // NaN: outside the reference's defined behaviour
    if (u < F.min_x || u > F.max_x) return q;          // :1218 inclusive bounds
    if (v < F.min_y || v > F.max_y) return q;          // :1220
    const int o = L.octave[i];                         // :1223
    if ((unsigned)o >= (unsigned)F.n_levels) return q; // the host checked it; never index past scale[]
    const float r = th * F.scale[o];                   // :1226
    q.in_view = 1;
    q.u = u;
    q.v = v;
    q.r = r;
    q.xr = u - mbf * invzc;                            // :1254
    q.cells = proj_cells(F, u, v, r, o);
    return q;
}

// the static gates of slot q: the level bounds of the mode, the window, then the stereo gate (:1252-1258)
RSCM_HD ProjStereoGate last_gate(const DevProjFrame& F, const float* u_right, const LpRec& q, int mode) {
    int lo, hi;
    last_levels(mode, ProjCells(q.cells).level, lo, hi);
    return ProjStereoGate{ProjGate(F, q.u, q.v, q.r, lo, hi), u_right, q.xr};
}

// :1242-1271 over the window of `q`: the feature slot i takes when the features with owner[f] < i are skipped, or -1
template <class OwnerPtr>
RSCM_HD int last_best(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP, int i,
                      OwnerPtr owner, int mode) {
    return proj_first_min(F, q.cells, dMP, i, owner, last_gate(F, u_right, q, mode), kLpThHigh);
}

// the cache of slot q: distance <= TH_HIGH on features without an entry occupant that has observations; true when
// more than four qualified
RSCM_HD bool last_candidates(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP,
                             const uint8_t* frame_occ, int mode, ProjCand& out) {
    return proj_candidates(F, q.cells, dMP, last_gate(F, u_right, q, mode),
                           [frame_occ](int f) { return frame_occ[f] == 2; }, kLpThHigh, out);
}

// What the rounds share, for LastFrame slot i: the window, the cache and an empty claim
RSCM_HD void last_setup_slot(const LastProjProblem& Q, int i, float th) {
    const DevProjFrame& F = *Q.F;
    LpRec q = lp_no_window();
    ProjCand cd = proj_no_cand();
    if (last_eligible(Q.L, i)) {
        q = last_setup(F, Q.mbf, Q.L, Q.Tcw, i, th);
        if (q.cells >= 0 && last_candidates(F, Q.u_right, q, Q.L.mp_desc[i], Q.frame_occ, Q.mode, cd))
            q.cells |= kProjMore;
    }
    Q.rec[i] = q;
    Q.cand[i] = cd;
    Q.claim[i] = -1;
}

// the matcher of the rounds (rsc_projrounds.h); lastproj.hip adds best_coop
struct LastRounds {
    static constexpr bool kCoopWalk = true;
    const LastProjProblem& Q;
    int mode;
    RSCM_HD int n_points() const { return Q.L.n; }
    RSCM_HD bool entry_occupied(int f) const { return Q.frame_occ[f] == 2; }
    RSCM_HD bool blocks(int i) const { return Q.L.mp_has_obs[i] != 0; }  // :1248-1250
    RSCM_HD int pick(int i, const int* owner) const {
        const int cells = Q.rec[i].cells;
        return cells < 0 ? kProjSkip : proj_pick(Q.cand[i], (cells & kProjMore) != 0, i, owner);
    }
    RSCM_HD int best(int i, const int* owner) const {  // :1242-1271
        return last_best(*Q.F, Q.u_right, Q.rec[i], Q.L.mp_desc[i], i, owner, mode);
    }
};

// :1278-1283 is proj_rot_bin(LastFrame angle, CurrentFrame angle).  The bins the removal of :1301-1311 spares,
// from the histogram over ALL claims
RSCM_HD void last_keep_bins(const int* hs, int keep[3]) { proj_keep_bins(hs, keep); }

#if defined(__HIPCC__)
// mid (may be NULL): recorded between the setup kernel and the rounds kernel.
hipError_t launch_search_by_projection_last(int count, int max_slots, const LastProjProblem* problems, float th,
                                            int check_orientation, hipEvent_t mid, hipStream_t st);
#endif

}  // namespace rsc
