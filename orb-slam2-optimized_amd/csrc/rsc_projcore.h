// rsc_projcore.h — what the sequentially greedy projection matchers share (rsc_frameproj.h, rsc_kfproj.h,
// rsc_localproj.h, rsc_lastproj.h), for the device and for the host emulations (tests/*proj_emu): the Frame /
// KeyFrame view, the window of GetFeaturesInArea (src/Frame.cpp:394-447, src/KeyFrame.cpp:560-604) and its walk,
// the static gates, the first-strict-minimum decision, the candidate cache and the rotation histogram.
//
// Window word.  proj_cells packs the cell range of one point as minX | maxX << 6 | minY << 12 | maxY << 18 |
// level << 24; kProjMore (bit 30) is set by the setup kernels when the cache below is not the whole list.
//
// Visiting order.  proj_walk visits the features of a window as the reference does: columns ix ascending, rows
// iy ascending, each cell's vector front to back (the CSR keeps mGrid's order).  Every decision here is "the
// first minimum under a strict <", so the visiting order IS the tie-break: it is the contract of this file.
//
// Candidate cache.  proj_candidates keeps the four smallest (distance, visiting order) candidates that pass the
// gates which do not depend on the claims (window, levels, stereo, not occupied on entry) and have distance <=
// keep_max.  keep_max is chosen per matcher so that a dropped candidate can change no decision; every kept
// candidate sorts before every dropped one, so the cache is a prefix of the sorted list and the first free
// entries of the cache are the first free entries of the walk.  When the prefix is used up and the list was
// longer, the window is walked again.
//
// Rounds.  One workgroup per problem iterates (proj_rounds in rsc_projrounds.h, emu_rounds in
// tests/proj_emu_common.h)
//     A[i] = decision of point i over its candidates f with owner[f] >= i
// where owner[f] = min{ j : A[j] == f, j blocks }, kProjOccupied for a feature occupied on entry and kProjFree
// for an unclaimed one.  Round r + 1 reads the A of round r.  Point i reads only the claims of points j < i
// (owner[f] < i can only come from such a j), so point 0 is final after round 1; once points 0..i-1 are final,
// point i sees exactly the sequential loop's free set, so points 0..i are final after round i + 1.  The fixed
// point is therefore unique, equals the sequential result, and is reached in at most n_eligible + 1 rounds (the
// last one only confirms): a plain bounded loop, no cross-workgroup hand-off, nothing to wait for.  Two owner
// rules: every claimer blocks (frame, keyframe: the reference skips any feature that has a MapPoint), or only
// claimers with Observations() > 0 block (local, last: a feature taken by a point without observations is
// taken again and overwritten; its claimers in point order are non-blocking points, then at most one blocking).
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include "rsc_math.h"

namespace rsc {

constexpr int kProjGridCols = 64, kProjGridRows = 48;  // FRAME_GRID_COLS / ROWS (Frame.hpp:20-21)
constexpr int kProjHistoLength = 30;                   // ORBmatcher::HISTO_LENGTH
constexpr int kProjMaxFeatures = 8192;                 // Frame::N bound (the LDS owner table)
constexpr int kProjFree = INT_MAX;                     // owner[f] of an unclaimed feature
constexpr int kProjOccupied = -1;                      // owner[f] of a pre-occupied feature
constexpr int kProjMore = 1 << 30;  // more than four candidates qualified: ProjCand is not the whole list
constexpr int kProjSkip = -3;       // a round's pick for a point without a window: it never claims

struct alignas(16) ProjDesc { uint32_t w[8]; };
struct alignas(8) ProjPt { float x, y; };

// the Frame or KeyFrame whose features the matcher walks
struct DevProjFrame {
    const ProjPt* kp;           // [n] mvKeysUn[i].pt
    const int32_t* octave;      // [n]
    const float* angle;         // [n] mvKeysUn[i].angle; NULL where no rotation check reads it (KeyFrame views)
    const ProjDesc* desc;       // [n] mDescriptors rows
    const int32_t* cell_begin;  // [64*48 + 1] mGrid as CSR, cell = ix * 48 + iy
    const int32_t* cell_feat;
    const float* scale;         // [n_levels] mvScaleFactors
    float min_x, max_x, min_y, max_y, gw_inv, gh_inv, fx, fy, cx, cy, log_sf;
    int n, n_levels;
};

// the best candidates of one point, ascending in (distance, visiting order): dist << 16 | feature, -1 = none
struct alignas(16) ProjCand { int32_t c[4]; };

RSCM_HD ProjCand proj_no_cand() {
    ProjCand cd;
    cd.c[0] = cd.c[1] = cd.c[2] = cd.c[3] = -1;
    return cd;
}

RSCM_HD int proj_desc_dist(const ProjDesc& a, const ProjDesc& b) {
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += __builtin_popcount(a.w[k] ^ b.w[k]);
    return d;
}

struct ProjCells {
    int x0, x1, y0, y1, level;
    RSCM_HD explicit ProjCells(int cells)
        : x0(cells & 63), x1((cells >> 6) & 63), y0((cells >> 12) & 63), y1((cells >> 18) & 63),
          level((cells >> 24) & 63) {}
};

// The cell range of GetFeaturesInArea (Frame.cpp:399-413, KeyFrame.cpp:565-579) as the window word, -1 when
// the window misses the grid.  level must be in [0, 64).
RSCM_HD int proj_cells(const DevProjFrame& F, float u, float v, float r, int level) {
    int x0 = (int)floorf((u - F.min_x - r) * F.gw_inv);
    if (x0 < 0) x0 = 0;
    if (x0 >= kProjGridCols) return -1;
    int x1 = (int)ceilf((u - F.min_x + r) * F.gw_inv);
    if (x1 > kProjGridCols - 1) x1 = kProjGridCols - 1;
    if (x1 < 0) return -1;
    int y0 = (int)floorf((v - F.min_y - r) * F.gh_inv);
    if (y0 < 0) y0 = 0;
    if (y0 >= kProjGridRows) return -1;
    int y1 = (int)ceilf((v - F.min_y + r) * F.gh_inv);
    if (y1 > kProjGridRows - 1) y1 = kProjGridRows - 1;
    if (y1 < 0) return -1;
    return x0 | x1 << 6 | y0 << 12 | y1 << 18 | level << 24;
}

// visit(f) for every feature of the window, in the reference's visiting order
template <class Visit>
RSCM_HD void proj_walk(const DevProjFrame& F, const ProjCells& w, Visit visit) {
    const int32_t* cell_begin = F.cell_begin;
    const int32_t* cell_feat = F.cell_feat;
    for (int ix = w.x0; ix <= w.x1; ++ix)
        for (int iy = w.y0; iy <= w.y1; ++iy) {
            const int c = ix * kProjGridRows + iy;
            const int e1 = cell_begin[c + 1];
            for (int e = cell_begin[c]; e < e1; ++e) visit(cell_feat[e]);
        }
}

// the strict window of GetFeaturesInArea (Frame.cpp:436-441, KeyFrame.cpp:589-593)
RSCM_HD bool proj_window_gate(const ProjPt* pts, float u, float v, float r, int f) {
    const ProjPt kp = pts[f];
    return fabsf(kp.x - u) < r && fabsf(kp.y - v) < r;
}

// the stereo gate (ORBmatcher.cpp:62-67, :1252-1258): a feature with a right coordinate must have it within r
// of the point's (strict >)
RSCM_HD bool proj_stereo_gate(const float* u_right, float xr, float r, int f) {
    const float ur = u_right[f];
    return !(ur > 0.0f && fabsf(xr - ur) > r);
}

// The gates of one (point, feature) pair that do not depend on the claims: octave in [lo, hi] and the window;
// with the stereo gate for the matchers that have it.  The gate holds the Frame's two arrays, not the Frame:
// through a reference the array pointers were loaded again for every feature of the walk.
struct ProjGate {
    const int32_t* octave;
    const ProjPt* kp;
    float u, v, r;
    int lo, hi;
    RSCM_HD ProjGate(const DevProjFrame& F, float u, float v, float r, int lo, int hi)
        : octave(F.octave), kp(F.kp), u(u), v(v), r(r), lo(lo), hi(hi) {}
    RSCM_HD bool operator()(int f) const {
        const int oct = octave[f];
        return oct >= lo && oct <= hi && proj_window_gate(kp, u, v, r, f);
    }
};
struct ProjStereoGate {
    ProjGate g;
    const float* u_right;
    float xr;
    RSCM_HD bool operator()(int f) const { return g(f) && proj_stereo_gate(u_right, xr, g.r, f); }
};

// ProjDesc / ProjCand / record parameters below are taken BY VALUE: the callers hand in elements of arrays in
// global memory, and a copy is one vector load where a reference is a load at every use.

// The feature point i takes over the window when the features with owner[f] < i are not available
// (pre-occupied features carry kProjOccupied): the first strict minimum of the descriptor distance, kept if
// <= cutoff; else -1.  bestDist starts at 256.
template <class OwnerPtr, class Gate>
RSCM_HD int proj_first_min(const DevProjFrame& F, int cells, const ProjDesc dMP, int i, OwnerPtr owner,
                           const Gate& gate, int cutoff) {
    if (cells < 0) return -1;
    const ProjDesc* desc = F.desc;
    int bestDist = 256, bestIdx = -1;
    proj_walk(F, ProjCells(cells), [&](int f) {
        if (!gate(f) || owner[f] < i) return;
        const int dist = proj_desc_dist(dMP, desc[f]);
        if (dist < bestDist) {
            bestDist = dist;
            bestIdx = f;
        }
    });
    return bestDist <= cutoff ? bestIdx : -1;
}

// the four smallest (distance, visiting order) of a stream
struct ProjTop4 {
    int k0 = INT_MAX, k1 = INT_MAX, k2 = INT_MAX, k3 = INT_MAX, count = 0;
    RSCM_HD void push(int dist, int f) {
        ++count;
        const int key = dist << 16 | f;  // a strict < keeps equal distances in visiting order
        if (dist < (k0 >> 16)) { k3 = k2; k2 = k1; k1 = k0; k0 = key; }
        else if (dist < (k1 >> 16)) { k3 = k2; k2 = k1; k1 = key; }
        else if (dist < (k2 >> 16)) { k3 = k2; k2 = key; }
        else if (dist < (k3 >> 16)) { k3 = key; }
    }
    RSCM_HD void store(ProjCand& out) const {
        out.c[0] = k0 == INT_MAX ? -1 : k0;
        out.c[1] = k1 == INT_MAX ? -1 : k1;
        out.c[2] = k2 == INT_MAX ? -1 : k2;
        out.c[3] = k3 == INT_MAX ? -1 : k3;
    }
};

// The walk once, for all rounds: the cache of the candidates that pass `gate`, are not entry_occupied(f) and
// have distance <= keep_max (< 32768).  Returns true when more than four qualified.
template <class Gate, class Occupied>
RSCM_HD bool proj_candidates(const DevProjFrame& F, int cells, const ProjDesc dMP, const Gate& gate,
                             Occupied entry_occupied, int keep_max, ProjCand& out) {
    const ProjDesc* desc = F.desc;
    ProjTop4 t;
    proj_walk(F, ProjCells(cells), [&](int f) {
        if (!gate(f) || entry_occupied(f)) return;
        const int dist = proj_desc_dist(dMP, desc[f]);
        if (dist <= keep_max) t.push(dist, f);
    });
    t.store(out);
    return t.count > 4;
}

// One round's choice from the cached candidates under "first free minimum": the feature, -1 for none, or -2
// when all four are taken by lower points and the list was longer (the window is then walked).
template <class OwnerPtr>
RSCM_HD int proj_pick(const ProjCand cd, bool more, int i, OwnerPtr owner) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = cd.c[k];
        if (c < 0) return -1;
        const int f = c & 0xffff;
        if (owner[f] >= i) return f;
    }
    return more ? -2 : -1;
}

// ORBmatcher.cpp:1407-1412, :1278-1283
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

// the bins the removal loops (:1430-1440, :1301-1311) spare
RSCM_HD void proj_keep_bins(const int* hs, int keep[3]) {
    const int m = proj_three_maxima(hs, kProjHistoLength);
    keep[0] = (m & 255) - 1;
    keep[1] = ((m >> 8) & 255) - 1;
    keep[2] = ((m >> 16) & 255) - 1;
}

}  // namespace rsc
