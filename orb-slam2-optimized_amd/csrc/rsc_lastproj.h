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
// visual-odometry points of UpdateLastFrame) takes a feature and blocks nobody, so
//     f is skipped by point i  <=>  min{ j : A[j] == f, has_obs[j] } < i
// with kProjOccupied for an entry occupant with observations.  The decision is "first free minimum, then
// cutoff" as in rsc_frameproj.h.  Fixed point: one workgroup per problem iterates
//     A[i] = first free minimum of point i's candidates f with owner[f] >= i   (kept if <= TH_HIGH)
// Point i reads only the claims of points j < i, so point 0 is final after round 1 and points 0..i after round
// i + 1: the fixed point is unique, equals the sequential result and is reached in at most n_eligible + 1
// rounds (the last one only confirms).  A plain bounded loop: no cross-workgroup hand-off, nothing to wait for.
//
// Candidate cache: the four smallest (distance, visiting order) candidates with distance <= TH_HIGH on
// features without an entry occupant that has observations.  TH_HIGH IS a sound filter here, unlike in
// rsc_localproj.h: the point takes its minimum over the free features first and applies the cutoff
// afterwards, and there is no runner-up test.  If the free minimum is above TH_HIGH the point claims nothing,
// and so it does when every free candidate was dropped; if it is <= TH_HIGH it was kept, and every kept
// candidate sorts before every dropped one.  When all four cached candidates are taken by lower slots and
// there were more, the window is walked again (last_best; on the device by 16 lanes, last_best_coop).
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
    LpRec q;
    q.u = q.v = q.r = q.xr = 0.0f;
    q.cells = -1;
    q.in_view = 0;
    q.pad[0] = q.pad[1] = 0;
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
    int x0 = (int)floorf((u - F.min_x - r) * F.gw_inv);
    if (x0 < 0) x0 = 0;
    if (x0 >= kProjGridCols) return q;
    int x1 = (int)ceilf((u - F.min_x + r) * F.gw_inv);
    if (x1 > kProjGridCols - 1) x1 = kProjGridCols - 1;
    if (x1 < 0) return q;
    int y0 = (int)floorf((v - F.min_y - r) * F.gh_inv);
    if (y0 < 0) y0 = 0;
    if (y0 >= kProjGridRows) return q;
    int y1 = (int)ceilf((v - F.min_y + r) * F.gh_inv);
    if (y1 > kProjGridRows - 1) y1 = kProjGridRows - 1;
    if (y1 < 0) return q;
    q.cells = x0 | x1 << 6 | y0 << 12 | y1 << 18 | o << 24;
    return q;
}

// The gates of one (point, feature) pair that do not depend on the claims: the level bounds and the strict
// window of GetFeaturesInArea (Frame.cpp:428-441), then the stereo gate (:1252-1258)
RSCM_HD bool last_static_gate(const DevProjFrame& F, const float* u_right, const LpRec& q, int lo, int hi, int f) {
    const int oct = F.octave[f];
    if (oct < lo || oct > hi) return false;
    const ProjPt kp = F.kp[f];
    if (!(fabsf(kp.x - q.u) < q.r && fabsf(kp.y - q.v) < q.r)) return false;
    const float ur = u_right[f];
    if (ur > 0.0f) {                        // :1252
        const float er = fabsf(q.xr - ur);  // :1255
        if (er > q.r) return false;         // :1256, strict
    }
    return true;
}

// :1242-1271 over the window of `q`: the feature point i takes when the features with owner[f] < i are skipped
// (an entry occupant with observations carries kProjOccupied), or -1
template <class OwnerPtr>
RSCM_HD int last_best(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP, int i,
                      OwnerPtr owner, int mode) {
    if (q.cells < 0) return -1;
    const int x0 = q.cells & 63, x1 = (q.cells >> 6) & 63, y0 = (q.cells >> 12) & 63, y1 = (q.cells >> 18) & 63;
    int lo, hi;
    last_levels(mode, (q.cells >> 24) & 63, lo, hi);
    int bestDist = 256, bestIdx = -1;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy) {
            const int c = ix * kProjGridRows + iy;
            const int e1 = F.cell_begin[c + 1];
            for (int e = F.cell_begin[c]; e < e1; ++e) {
                const int f = F.cell_feat[e];
                if (!last_static_gate(F, u_right, q, lo, hi, f)) continue;
                if (owner[f] < i) continue;  // :1248-1250
                const int dist = proj_desc_dist(dMP, F.desc[f]);
                if (dist < bestDist) {       // :1264
                    bestDist = dist;
                    bestIdx = f;
                }
            }
        }
    return bestDist <= kLpThHigh ? bestIdx : -1;  // :1271
}

// The walk of last_best once, for all rounds: the four smallest (distance, visiting order) among the
// candidates with distance <= TH_HIGH on features without an entry occupant that has observations.  Returns
// true when more than four qualified.  One round's choice from the cache is proj_pick (rsc_frameproj.h).
RSCM_HD bool last_candidates(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP,
                             const uint8_t* frame_occ, int mode, ProjCand& out) {
    const int x0 = q.cells & 63, x1 = (q.cells >> 6) & 63, y0 = (q.cells >> 12) & 63, y1 = (q.cells >> 18) & 63;
    int lo, hi;
    last_levels(mode, (q.cells >> 24) & 63, lo, hi);
    int k0 = INT_MAX, k1 = INT_MAX, k2 = INT_MAX, k3 = INT_MAX, count = 0;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy) {
            const int c = ix * kProjGridRows + iy;
            const int e1 = F.cell_begin[c + 1];
            for (int e = F.cell_begin[c]; e < e1; ++e) {
                const int f = F.cell_feat[e];
                if (!last_static_gate(F, u_right, q, lo, hi, f)) continue;
                if (frame_occ[f] == 2) continue;
                const int dist = proj_desc_dist(dMP, F.desc[f]);
                if (dist > kLpThHigh) continue;
                ++count;
                const int key = dist << 16 | f;  // a strict < keeps equal distances in visiting order
                if (dist < (k0 >> 16)) { k3 = k2; k2 = k1; k1 = k0; k0 = key; }
                else if (dist < (k1 >> 16)) { k3 = k2; k2 = k1; k1 = key; }
                else if (dist < (k2 >> 16)) { k3 = k2; k2 = key; }
                else if (dist < (k3 >> 16)) { k3 = key; }
            }
        }
    out.c[0] = k0 == INT_MAX ? -1 : k0;
    out.c[1] = k1 == INT_MAX ? -1 : k1;
    out.c[2] = k2 == INT_MAX ? -1 : k2;
    out.c[3] = k3 == INT_MAX ? -1 : k3;
    return count > 4;
}

// :1278-1283 is proj_rot_bin(LastFrame angle, CurrentFrame angle); ComputeThreeMaxima is proj_three_maxima.
// The bins the removal of :1301-1311 spares, from the histogram over ALL claims
RSCM_HD void last_keep_bins(const int* hs, int keep[3]) {
    const int m = proj_three_maxima(hs, kProjHistoLength);
    keep[0] = (m & 255) - 1;
    keep[1] = ((m >> 8) & 255) - 1;
    keep[2] = ((m >> 16) & 255) - 1;
}

#if defined(__HIPCC__)
// mid (may be NULL): recorded between the setup kernel and the rounds kernel.
hipError_t launch_search_by_projection_last(int count, int max_slots, const LastProjProblem* problems, float th,
                                            int check_orientation, hipEvent_t mid, hipStream_t st);
#endif

}  // namespace rsc
