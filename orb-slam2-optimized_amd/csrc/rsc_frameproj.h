// rsc_frameproj.h — ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist)
// (src/ORBmatcher.cpp:1317-1444 with Frame::GetFeaturesInArea, src/Frame.cpp:394-447): device layout
// and the per-MapPoint arithmetic, shared by frameproj.hip and the host emulation (tests/frameproj_emu).
//
// The matcher is sequentially greedy: MapPoint i skips the Frame features that earlier MapPoints
// claimed (:1386-1387).  Mapping: one workgroup per (Frame, KeyFrame) problem iterates to the fixed
// point of
//     A[i] = first minimum descriptor distance over the candidates f of MapPoint i that are not
//            pre-occupied and whose owner[f] = min{ j : A[j] == f } is >= i   (kept if <= ORBdist)
// Round r + 1 reads the A of round r (owner table in LDS, built with atomicMin).  MapPoint 0 never
// sees an owner below it, so it is final after round 1; once slots 0..i-1 are final, every feature
// they hold has an owner < i and slot i sees exactly the sequential loop's free set, so slots 0..i are
// final after round i + 1.  The fixed point is therefore unique, equals the sequential result, and is
// reached in at most n_eligible + 1 rounds (the last one only confirms): a plain bounded loop, no
// cross-workgroup hand-off, nothing to wait for.  Candidates are visited in the reference's (ix, iy,
// cell order) order with a strict `<`, so the first minimum is the reference's bestIdx2.
//
// Float conventions are those of oracle/sim3match_oracle.h (rows summed left to right, invz through a
// double division, logf as the float rounding of dm::log); what differs from SearchBySim3 is stated
// at each line.  Precondition: no eligible MapPoint has camera z == 0 (the reference feeds NaN to
// floor there); such a point is skipped.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include "rsc_math.h"

namespace rsc {

constexpr int kProjGridCols = 64, kProjGridRows = 48;  // FRAME_GRID_COLS / ROWS (Frame.hpp:20-21)
constexpr int kProjHistoLength = 30;                   // ORBmatcher::HISTO_LENGTH
constexpr int kProjMaxFeatures = 8192;                 // Frame::N bound (the LDS owner table)
constexpr int kProjThreads = 512;
constexpr int kProjFree = INT_MAX;                     // owner[f] of an unclaimed feature
constexpr int kProjOccupied = -1;                      // owner[f] of a pre-occupied feature

struct alignas(16) ProjDesc { uint32_t w[8]; };
struct alignas(8) ProjPt { float x, y; };

// the current Frame as the matcher reads it
struct DevProjFrame {
    const ProjPt* kp;           // [n] mvKeysUn[i].pt
    const int32_t* octave;      // [n]
    const float* angle;         // [n] mvKeysUn[i].angle
    const ProjDesc* desc;       // [n] mDescriptors rows
    const int32_t* cell_begin;  // [64*48 + 1] mGrid as CSR, cell = ix * 48 + iy
    const int32_t* cell_feat;
    const float* scale;         // [n_levels] mvScaleFactors
    float min_x, max_x, min_y, max_y, gw_inv, gh_inv, fx, fy, cx, cy, log_sf;
    int n, n_levels;
};

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
constexpr int kProjMore = 1 << 30;  // more than four candidates qualified: ProjCand is not the whole list

// the best candidates of one MapPoint, ascending in (distance, visiting order): dist << 16 | feature, -1 = none
struct alignas(16) ProjCand { int32_t c[4]; };

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

RSCM_HD int proj_desc_dist(const ProjDesc& a, const ProjDesc& b) {
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += __builtin_popcount(a.w[k] ^ b.w[k]);
    return d;
}

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
    ProjRec w;
    w.u = u;
    w.v = v;
    w.r = r;
    w.cells = x0 | x1 << 6 | y0 << 12 | y1 << 18 | level << 24;
    return w;
}

// :1380-1400 over the window of `q`: the feature MapPoint i takes when the features with
// owner[f] < i are not available (pre-occupied features carry kProjOccupied), or -1.
template <class OwnerPtr>
RSCM_HD int proj_best(const DevProjFrame& F, const ProjRec& q, const ProjDesc& dMP, int i, OwnerPtr owner,
                      int orb_dist) {
    if (q.cells < 0) return -1;
    const int x0 = q.cells & 63, x1 = (q.cells >> 6) & 63, y0 = (q.cells >> 12) & 63, y1 = (q.cells >> 18) & 63;
    const int level = (q.cells >> 24) & 63;
    int bestDist = 256, bestIdx = -1;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy) {
            const int c = ix * kProjGridRows + iy;
            const int e1 = F.cell_begin[c + 1];
            for (int e = F.cell_begin[c]; e < e1; ++e) {
                const int f = F.cell_feat[e];
                const int oct = F.octave[f];
                if (oct < level - 1 || oct > level + 1) continue;  // [L-1, L+1], bCheckLevels true
                const ProjPt kp = F.kp[f];
                if (!(fabsf(kp.x - q.u) < q.r && fabsf(kp.y - q.v) < q.r)) continue;
                if (owner[f] < i) continue;  // mvpMapPoints[i2] set (:1386): before the call or by j < i
                const int dist = proj_desc_dist(dMP, F.desc[f]);
                if (dist < bestDist) {
                    bestDist = dist;
                    bestIdx = f;
                }
            }
        }
    return bestDist <= orb_dist ? bestIdx : -1;
}

// The walk of proj_best once, for all rounds: the four smallest (distance, visiting order) among the
// candidates with distance <= ORBdist on features that are free before the call.  Returns true when more
// than four qualified.
RSCM_HD bool proj_candidates(const DevProjFrame& F, const ProjRec& q, const ProjDesc& dMP, const int32_t* frame_mp,
                             int orb_dist, ProjCand& out) {
    const int x0 = q.cells & 63, x1 = (q.cells >> 6) & 63, y0 = (q.cells >> 12) & 63, y1 = (q.cells >> 18) & 63;
    const int level = (q.cells >> 24) & 63;
    int k0 = INT_MAX, k1 = INT_MAX, k2 = INT_MAX, k3 = INT_MAX, count = 0;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy) {
            const int c = ix * kProjGridRows + iy;
            const int e1 = F.cell_begin[c + 1];
            for (int e = F.cell_begin[c]; e < e1; ++e) {
                const int f = F.cell_feat[e];
                const int oct = F.octave[f];
                if (oct < level - 1 || oct > level + 1) continue;
                const ProjPt kp = F.kp[f];
                if (!(fabsf(kp.x - q.u) < q.r && fabsf(kp.y - q.v) < q.r)) continue;
                if (frame_mp[f] >= 0) continue;
                const int dist = proj_desc_dist(dMP, F.desc[f]);
                if (dist > orb_dist || dist >= 256) continue;
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

// One round's choice from the cached candidates: the feature, -1 for none, or -2 when all four are taken
// by lower slots and the list was longer (proj_best then walks the window).
template <class OwnerPtr>
RSCM_HD int proj_pick(const ProjCand& cd, bool more, int i, OwnerPtr owner) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = cd.c[k];
        if (c < 0) return -1;
        const int f = c & 0xffff;
        if (owner[f] >= i) return f;
    }
    return more ? -2 : -1;
}

// :1407-1412
RSCM_HD int proj_rot_bin(float angle_kf, float angle_frame) {
    const float factor = 1.0f / (float)kProjHistoLength;
    float rot = angle_kf - angle_frame;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == kProjHistoLength) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cpp:1446-1487) on the bin sizes, as orbmatch.hip runs it
// (returns (ind1 + 1) | (ind2 + 1) << 8 | (ind3 + 1) << 16)
RSCM_HD int proj_three_maxima(const int* hs, int L) {
    int max1 = 0, max2 = 0, max3 = 0;
    int ind1 = -1, ind2 = -1, ind3 = -1;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const int s = hs[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s; ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
    return (ind1 + 1) | (ind2 + 1) << 8 | (ind3 + 1) << 16;
}

#if defined(__HIPCC__)
hipError_t launch_search_by_projection(int count, int max_kf_points, const FrameProjProblem* problems, float th,
                                       int orb_dist, int check_orientation, hipStream_t st);
#endif

}  // namespace rsc
