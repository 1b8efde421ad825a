// rsc_stereo.h — Frame::ComputeStereoMatches() (src/Frame.cpp:538-673, the keypoint-only matcher of this fork)
// over a batch of (resident left Frame view, right features) records: device layout and the arithmetic of one
// left keypoint and of the cut, shared by stereo.hip and the host emulation (tests/stereo_emu).
//
// The function as the reference has it, for a left keypoint i with uL, yL = mvKeysUn[i].pt, levelL its octave:
//   maxD       mbf / mb, a float division; minU = uL - maxD, maxU = uL; maxU < 0 skips the keypoint (:565)
//   window     the right keypoints, sorted by (pt.y, index), between two binary searches with <= (:569-610):
//              r = 2.0f * mvScaleFactors[levelL], those with y > yL - r and y <= yL + r (lower edge out, upper edge
//              in); yL -/+ r is a multiply then an add, each rounded.  -0.0f == +0.0f in the sort and the searches
//   candidate  octaveR in [levelL - 1, levelL + 1], uR >= minU && uR <= maxU (:623-627); left is mvKeysUn /
//              mDescriptors, right is mvKeysRight (as extracted) / mDescriptorsRight
//   best       bestDist starts at TH_HIGH = 100, strict <, in sorted order (:632): the winner is the candidate with
//              the smallest (distance, y, index); it is accepted when bestDist < (TH_HIGH + TH_LOW) / 2 = 75
//   finish     disparity = uL - best_uR, kept when 0 <= disparity < maxD; disparity <= 0 becomes (float)0.01 and
//              mvuRight = (float)((double)uL - 0.01); mvDepth = mbf / disparity (:643-654)
//   cut        vDistIdx sorted by (dist, i), median = vDistIdx[size / 2].first, thDist = 1.5f * 1.4f * median in
//              float; every entry with (float)dist >= thDist goes back to -1 / -1 (:659-672).  A median of 0
//              removes every match
// No sort is made here.  The window is two float comparisons per right keypoint; the sorted-order tie-break is the
// 64-bit key dist << 45 | order(y) << 13 | index, whose minimum over any partition of the candidates is the
// reference's winner (stm_key).  The median is the smallest d whose cumulative count over a histogram of the
// accepted distances exceeds size / 2, and the back-walk over the sorted list is "every accepted entry at or above
// thDist" (stm_cut_*).
//
// Pinned where the reference is undefined: with no accepted match it reads vDistIdx[0] of an empty vector and its
// loop does nothing; here nothing is removed, median = -1 and th_dist = 1.5f * 1.4f * -1.  It reads mb before
// the constructor assigns it (:130 against :157), so mb is an argument.  A negative scale factor makes the
// reference's uint16_t loop run past the list (.at() throws); here such a keypoint has an empty window.
#pragma once
#include "rsc_projcore.h"

#ifndef RSC_STEREO_MAX_RIGHT  // include/rsc.h
#define RSC_STEREO_MAX_RIGHT 8192
#endif

namespace rsc {

constexpr int kStmMaxRight = RSC_STEREO_MAX_RIGHT;
constexpr int kStmThreads = 256;               // match kernel: four waves, one left keypoint per wave at a time
constexpr int kStmWaves = kStmThreads / 64;
constexpr int kStmPerWave = 8;                 // left keypoints of one wave
constexpr int kStmTile = kStmWaves * kStmPerWave;  // left keypoints of one workgroup
constexpr int kStmChunk = 2048;                // right keypoints staged in LDS at a time: (y, u, octave), 24 KB
constexpr int kStmThHigh = 100, kStmThLow = 50;            // ORBmatcher::TH_HIGH, TH_LOW
constexpr int kStmThOrbDist = (kStmThHigh + kStmThLow) / 2;  // 75
constexpr int kStmCutThreads = 256;            // cut kernel: one workgroup per frame
constexpr unsigned long long kStmNoKey = ~0ull;
static_assert(kStmMaxRight <= (1 << 13), "13 index bits in the key");

struct StereoOut {  // rsc_stereo_result
    int32_t n_candidates, n_removed, median;
    float th_dist;
};

struct StereoProblem {
    const DevProjFrame* left;  // the resident view's header: kp, octave, desc, scale
    const ProjPt* r_kp;        // [n_right] mvKeysRight[i].pt
    const int32_t* r_octave;   // [n_right]
    const ProjDesc* r_desc;    // [n_right] mDescriptorsRight rows
    float* u_right;            // [n_left] mvuRight
    float* depth;              // [n_left] mvDepth
    int32_t* best_right;       // [n_left] matched right index before the cut, -1: none accepted
    int32_t* best_dist;        // [n_left] its distance, -1: none accepted
    float* view_uright;        // the view's own mvuRight (set_stereo), or NULL
    StereoOut* result;
    int32_t n_left, n_right;
    float mbf, mb;
};

// the gates of one left keypoint, which no right keypoint changes
struct StereoLeft {
    float uL, lo, hi, minU, maxU;
    int level;
    bool live;  // :565
};

RSCM_HD float stm_max_d(float mbf, float mb) { return mbf / mb; }

RSCM_HD StereoLeft stm_left(const ProjPt& kp, int level, float scale, float maxD) {
    StereoLeft L;
    L.uL = kp.x;
    L.minU = kp.x - maxD;
    L.maxU = kp.x - 0.0f;  // minD = 0 (:552, :563)
    const float r = 2.0f * scale;
    L.lo = kp.y - r;
    L.hi = kp.y + r;
    L.level = level;
    L.live = !(L.maxU < 0.0f);
    return L;
}

// the window, the octave gate and the u gate of one right keypoint (:569-627)
RSCM_HD bool stm_gate(const StereoLeft& L, float yR, float uR, int octR) {
    return yR > L.lo && yR <= L.hi && !(octR < L.level - 1 || octR > L.level + 1) && uR >= L.minU && uR <= L.maxU;
}

// a float as an unsigned word of the same order, both zeros alike
RSCM_HD uint32_t stm_order(float y) {
    if (y == 0.0f) y = 0.0f;
    uint32_t b;
    __builtin_memcpy(&b, &y, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// bestDist starts at TH_HIGH under a strict <: a candidate at 100 or above never becomes the best
RSCM_HD unsigned long long stm_key(int dist, float yR, int idx) {
    if (dist >= kStmThHigh) return kStmNoKey;
    return (unsigned long long)dist << 45 | (unsigned long long)stm_order(yR) << 13 | (unsigned long long)idx;
}
RSCM_HD int stm_key_dist(unsigned long long key) { return (int)(key >> 45); }
RSCM_HD int stm_key_idx(unsigned long long key) { return (int)(key & 0x1fffu); }

// :640-655 for the winner of left keypoint i; best_uR is read only when the distance passes
RSCM_HD void stm_finish(const StereoProblem& P, int i, const StereoLeft& L, float maxD, unsigned long long key) {
    float u = -1.0f, z = -1.0f;
    int br = -1, bd = -1;
    if (key != kStmNoKey && stm_key_dist(key) < kStmThOrbDist) {
        const int idx = stm_key_idx(key);
        const float best_uR = P.r_kp[idx].x;
        float disparity = L.uL - best_uR;
        if (disparity >= 0.0f && disparity < maxD) {
            u = best_uR;
            if (disparity <= 0.0f) {
                disparity = (float)0.01;
                u = (float)((double)L.uL - 0.01);
            }
            z = P.mbf / disparity;
            br = idx;
            bd = stm_key_dist(key);
        }
    }
    P.u_right[i] = u;
    P.depth[i] = z;
    P.best_right[i] = br;
    P.best_dist[i] = bd;
}

// :659-661 from the histogram of the accepted distances: vDistIdx[size / 2].first is the smallest d with more
// than size / 2 entries at or below it
RSCM_HD StereoOut stm_cut_threshold(const int* hist) {
    StereoOut o;
    int size = 0;
    for (int d = 0; d < kStmThOrbDist; ++d) size += hist[d];
    o.n_candidates = size;
    o.n_removed = 0;
    o.median = -1;
    if (size > 0) {
        int cum = 0;
        for (int d = 0; d < kStmThOrbDist; ++d) {
            cum += hist[d];
            if (cum > size / 2) {
                o.median = d;
                break;
            }
        }
    }
    const float median = (float)o.median;
    o.th_dist = 1.5f * 1.4f * median;
    return o;
}

// :663-672: an accepted entry at or above thDist is reset
RSCM_HD bool stm_cut_removes(const StereoOut& o, int dist) {
    return o.n_candidates > 0 && dist >= 0 && !((float)dist < o.th_dist);
}

#if defined(__HIPCC__)
// one launch per phase for `count` frames: the match kernel over (tiles of the longest left frame) x count
// workgroups, then the cut kernel, one workgroup per frame; `mid` (may be NULL) is recorded between them
hipError_t launch_stereo(const StereoProblem* problems, int count, int max_left, hipEvent_t mid, hipStream_t st);
#endif

}  // namespace rsc
