// rsc_triang.h — LocalMapping::CreateNewMapPoints' matcher and geometry on the GPU:
// ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:489-669) and the per-pair triangulation
// (src/LocalMapping.cpp:262-407).  Device layout, the per-candidate and per-pair functions (RSC_HD: the
// kernels of triang.hip and the host emulation of tests/triang_emu run the same text) and the launchers.
//
// Independence.  vbMatched2 (:509) is read at :567 and never set, so a KeyFrame-1 slot's winner depends on
// no other slot: every (common node, eligible KeyFrame-1 slot) is one independent item, and two slots may
// take the same KeyFrame-2 feature (the reference then creates two MapPoints on it).  The winner of a slot is
// the smallest distance among the candidates that pass the geometry, ties to the later position in the
// node's vector: `dist > bestDist` skips, so an equal distance goes on and, accepted, replaces (:580-601).
//
// Kernels of one matcher launch:
//  0. tri_join_kernel — one workgroup per problem: the node ids both FeatureVectors hold (binary search, as
//     bow_join_kernel), and for each the eligible KeyFrame-1 slots as items (FeatureVector entry, b0, nb) in
//     three classes by the KeyFrame-2 node size nb (<= 16, <= 128, larger); also clears the outputs.  Eligible:
//     the slot's skip flag is clear; the host sets it for a MapPoint and, under bOnlyStereo, for mvuRight < 0.
//  1. tri_match_kernel — a group of 4 / 16 / 64 lanes per item strides the node's KeyFrame-2 features and
//     reduces one packed key (distance << 16 | 0xFFFF - position); lane 0 writes the slot's match.  An item
//     whose line has den == 0 raises the slot's flag and the problem's den_zero word instead.
//  2. tri_finish_kernel — one workgroup per problem: den_zero empties the result (`return false`, :552-553);
//     else the orientation mask (when on) and the count.
// and tri_pairs_kernel: one lane per matched pair, the whole of :262-407.
//
// Arithmetic: float expressions as written, sums left to right, no contraction; the double comparisons of
// :597 / :293 / :350-387 in double.  The float 4x4 JacobiSVD is Eigen's two-sided Jacobi restated as the
// double 3x3 form of rsc_mlpnp.h (parity with an Eigen build unpinned).
#pragma once
#include <cmath>
#include <cstdint>
#include "rsc_core.h"

namespace rsc {

constexpr int kTriMaxFeatures = 8192;  // features per view (positions fit the key's 16 bits)
constexpr int kTriThLow = 50;          // ORBmatcher::TH_LOW
constexpr int kTriThreads = 256;       // join / match / finish workgroup
constexpr int kTriMatchGroups = 16;    // tri_match_kernel workgroups per problem
constexpr int kTriClasses = 3;
constexpr uint32_t kTriNoKey = 0xFFFFFFFFu;

// group width of an item's lanes by the KeyFrame-2 node size
RSC_HD int tri_class_of(int nb) { return nb <= 16 ? 0 : (nb <= 128 ? 1 : 2); }
RSC_HD int tri_class_width(int cls) { return cls == 0 ? 4 : (cls == 1 ? 16 : 64); }

// status of one pair: the `continue` it took (LocalMapping.cpp)
enum TriStatus : int32_t {
    kTriOk = 0,
    kTriSvdW0 = 1,        // temp(3) == 0                           :309
    kTriLowParallax = 2,  // no stereo and very low parallax        :326
    kTriBehind1 = 3,      // z1 <= 0                                :331
    kTriBehind2 = 4,      // z2 <= 0                                :335
    kTriReproj1 = 5,      // reprojection error in the current KeyFrame  :350 / :361
    kTriReproj2 = 6,      // reprojection error in the neighbour         :376 / :387
    kTriZeroDist = 7,     // dist1 == 0 || dist2 == 0               :398
    kTriScale = 8,        // scale consistency                      :406
};

// ---- the matcher's per-slot and per-candidate arithmetic --------------------------------------------

// Epipole of KeyFrame 1 in KeyFrame 2 (:496-502).  A zero or negative C2z is not special: the IEEE results
// flow through, and a NaN epipole skips nobody (every comparison with it is false).
RSC_HD void tri_epipole(const float* R2w, const float* t2w, const float* Cw, float fx, float fy, float cx, float cy,
                        float& ex, float& ey) {
    const float c0 = ((R2w[0] * Cw[0] + R2w[1] * Cw[1]) + R2w[2] * Cw[2]) + t2w[0];
    const float c1 = ((R2w[3] * Cw[0] + R2w[4] * Cw[1]) + R2w[5] * Cw[2]) + t2w[1];
    const float c2 = ((R2w[6] * Cw[0] + R2w[7] * Cw[1]) + R2w[8] * Cw[2]) + t2w[2];
    const float invz = 1.0f / c2;
    ex = (fx * c0) * invz + cx;
    ey = (fy * c1) * invz + cy;
}

// Epipolar line of kp1 in the second image, l = x1' F12 = [a b c] (:546-550); F row-major.
RSC_HD void tri_epiline(const float* F, float x, float y, float& a, float& b, float& c, float& den) {
    a = (x * F[0] + y * F[3]) + F[6];
    b = (x * F[1] + y * F[4]) + F[7];
    c = (x * F[2] + y * F[5]) + F[8];
    den = a * a + b * b;
}

// The geometry of one candidate whose distance passed `dist > TH_LOW || dist > bestDist` (:585-597).
// sf2 = mvScaleFactors[kp2.octave]; mvLevelSigma2 = sf2 * sf2 in float (ORBextractor.cpp:353-360).
RSC_HD bool tri_candidate_ok(float a, float b, float c, float den, float ex, float ey, bool stereo1, bool stereo2,
                             float x2, float y2, float sf2) {
    if (!stereo1 && !stereo2) {
        const float distex = ex - x2;
        const float distey = ey - y2;
        if (distex * distex + distey * distey < 100.0f * sf2) return false;  // :589 (int 100 -> float), strict
    }
    const float num = (a * x2 + b * y2) + c;
    const float dsqr = (num * num) / den;
    const float sigma2 = sf2 * sf2;
    return (double)dsqr < 3.84 * (double)sigma2;  // :597, in double
}

// key of an accepted candidate: smaller distance first, then the LATER position (an equal distance replaces)
RSC_HD uint32_t tri_key(uint32_t dist, uint32_t pos) { return (dist << 16) | (0xFFFFu - pos); }
RSC_HD uint32_t tri_key_pos(uint32_t key) { return 0xFFFFu - (key & 0xFFFFu); }

// Orientation bin (:612-618): the same expression as SearchByBoW's (bow_rot_bin, rsc_orbmatch.h).
RSC_HD int tri_rot_bin(float angle1, float angle2) {
    const float factor = 1.0f / 30.0f;
    float rot = angle1 - angle2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == 30) bin = 0;
    return bin;
}

// ComputeThreeMaxima (ORBmatcher.cpp:1446-1487) over the 30 bin counts hs(i)
struct TriMaxima { int ind1, ind2, ind3; };
template <class H>
RSC_HD TriMaxima tri_three_maxima(H hs) {
    int max1 = 0, max2 = 0, max3 = 0;
    int ind1 = -1, ind2 = -1, ind3 = -1;
    RSC_UNROLL for (int i = 0; i < 30; ++i) {
        const int s = hs(i);
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
    return TriMaxima{ind1, ind2, ind3};
}

// ---- the pair geometry ------------------------------------------------------------------------------

// One KeyFrame as the triangulation reads it.  Pointers: device memory in the kernels, host in the emulation.
struct TriView {
    const float* kp;          // [n][2] mvKeysUn[i].pt
    const float* kp_raw;      // [n][2] mvKeys[i].pt (UnprojectStereo, KeyFrame.cpp:611-612)
    const int32_t* octave;    // [n]
    const float* scale;       // [n_levels] mvScaleFactors
    const float* u_right;     // [n] mvuRight
    const float* depth;       // [n] mvDepth
    const float* cos_stereo;  // [n] cos(2*atan2(mb/2, mvDepth[i])), read only where mvuRight[i] >= 0
    float Rcw[9], tcw[3];     // Tcw
    float Rwc[9], Ow[3];      // Twc as KeyFrame::SetPose stored it (KeyFrame.cpp:64-66)
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    float scale_factor;       // mfScaleFactor
    int32_t n, n_levels;
};

RSC_HD float tri_dot3(const float* r, const float* x) { return (r[0] * x[0] + r[1] * x[1]) + r[2] * x[2]; }
RSC_HD float tri_norm3(const float* x) { return sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); }

// real_2x2_jacobi_svd (Eigen/src/SVD/JacobiSVD.h) in float: the left (cl, sl) and right (cr, sr) rotations of
// the 2x2 block (m00 m01; m10 m11); ml_jacobi_2x2 of rsc_mlpnp.h with float operands.
RSC_HD void tri_jacobi_2x2(float m00, float m01, float m10, float m11, float& cl, float& sl, float& cr, float& sr) {
    const float considerAsZero = lim<float>::min();
    const float t = m00 + m11;
    const float d = m10 - m01;
    const bool dz = rabs(d) < considerAsZero;
    const float u = t / d;
    const float tmp = sqrtf(1.0f + u * u);
    const float s1 = dz ? 0.0f : 1.0f / tmp;
    const float c1 = dz ? 1.0f : u / tmp;
    {
        const bool rot = !((c1 == 1.0f) && (s1 == 0.0f));
        const float x0 = m00, y0 = m10, x1 = m01, y1 = m11;
        m00 = rot ? c1 * x0 + s1 * y0 : x0;
        m10 = rot ? -s1 * x0 + c1 * y0 : y0;
        m01 = rot ? c1 * x1 + s1 * y1 : x1;
        m11 = rot ? -s1 * x1 + c1 * y1 : y1;
    }
    const float deno = 2.0f * rabs(m01);
    const bool nz = deno < considerAsZero;
    const float tau = (m00 - m11) / deno;
    const float w = sqrtf(tau * tau + 1.0f);
    const float tt = 1.0f / (tau > 0.0f ? tau + w : tau - w);
    const float sign_t = tt > 0.0f ? 1.0f : -1.0f;
    const float nn = 1.0f / sqrtf(tt * tt + 1.0f);
    sr = nz ? 0.0f : -sign_t * (m01 / rabs(m01)) * rabs(tt) * nn;
    cr = nz ? 1.0f : nn;
    const float crt = cr, srt = -sr;
    cl = c1 * crt - s1 * srt;
    sl = c1 * srt + s1 * crt;
}

// JacobiSVD<Matrix4f>(A, ComputeFullV).matrixV().rightCols<1>() (LocalMapping.cpp:303-307): square input, so
// no QR preconditioner; scaling by the largest absolute coefficient; sweeps over (p, q < p) until no
// off-diagonal pair exceeds max(min, 2 eps maxDiag); singular values |W(i,i)| * scale; descending selection
// sort (first maximum, stop at a zero maximum) swapping V's columns; the last column.  All in registers.
RSC_HD void tri_svd_last_v(const float (&A)[4][4], float (&v)[4]) {
    const float precision = 2.0f * lim<float>::eps();
    const float considerAsZero = lim<float>::min();
    float scale = rabs(A[0][0]);
    RSC_UNROLL for (int c = 0; c < 4; ++c)
        RSC_UNROLL for (int r = 0; r < 4; ++r) {
            if (r == 0 && c == 0) continue;
            // Eigen's maxCoeff visitor: a NaN never compares greater, the running maximum stays
            if (rabs(A[r][c]) > scale) scale = rabs(A[r][c]);
        }
    if (scale == 0.0f) scale = 1.0f;
    float W[4][4], V[4][4];
    RSC_UNROLL for (int r = 0; r < 4; ++r)
        RSC_UNROLL for (int c = 0; c < 4; ++c) {
            W[r][c] = A[r][c] / scale;
            V[r][c] = (r == c) ? 1.0f : 0.0f;
        }
    float maxDiag = rabs(W[0][0]);
    RSC_UNROLL for (int i = 1; i < 4; ++i) if (rabs(W[i][i]) > maxDiag) maxDiag = rabs(W[i][i]);
    bool finished = false;
    while (!finished) {
        finished = true;
        RSC_UNROLL for (int p = 1; p < 4; ++p) {
            RSC_UNROLL for (int q = 0; q < p; ++q) {
                const float pt = precision * maxDiag;
                const float threshold = (considerAsZero < pt) ? pt : considerAsZero;
                if (rabs(W[p][q]) > threshold || rabs(W[q][p]) > threshold) {
                    finished = false;
                    float cl, sl, cr, sr;
                    tri_jacobi_2x2(W[p][p], W[p][q], W[q][p], W[q][q], cl, sl, cr, sr);
                    const bool left = !(cl == 1.0f && sl == 0.0f);
                    RSC_UNROLL for (int c = 0; c < 4; ++c) {
                        const float xi = W[p][c], yi = W[q][c];
                        W[p][c] = left ? cl * xi + sl * yi : xi;
                        W[q][c] = left ? -sl * xi + cl * yi : yi;
                    }
                    const bool right = !(cr == 1.0f && sr == 0.0f);
                    RSC_UNROLL for (int r = 0; r < 4; ++r) {
                        const float xi = W[r][p], yi = W[r][q];
                        W[r][p] = right ? cr * xi - sr * yi : xi;
                        W[r][q] = right ? sr * xi + cr * yi : yi;
                    }
                    RSC_UNROLL for (int r = 0; r < 4; ++r) {
                        const float xi = V[r][p], yi = V[r][q];
                        V[r][p] = right ? cr * xi - sr * yi : xi;
                        V[r][q] = right ? sr * xi + cr * yi : yi;
                    }
                    const float a = rabs(W[p][p]), b = rabs(W[q][q]);
                    const float mm = (a < b) ? b : a;
                    maxDiag = (maxDiag < mm) ? mm : maxDiag;
                }
            }
        }
        RSC_LOOP_FENCE();
    }
    float sv[4];
    RSC_UNROLL for (int i = 0; i < 4; ++i) sv[i] = rabs(W[i][i]) * scale;
    bool stopped = false;
    RSC_UNROLL for (int i = 0; i < 4; ++i) {
        if (!stopped) {
            int pos = 0;
            float mv = sv[i];
            RSC_UNROLL for (int j = 1; j < 4 - i; ++j) {
                const bool gt = sv[i + j] > mv;
                mv = gt ? sv[i + j] : mv;
                pos = gt ? j : pos;
            }
            if (mv == 0.0f) {
                stopped = true;
            } else {
                RSC_UNROLL for (int j = 1; j < 4 - i; ++j) {
                    const bool sw = (j == pos);
                    const float a = sv[i], b = sv[i + j];
                    sv[i] = sw ? b : a;
                    sv[i + j] = sw ? a : b;
                    RSC_UNROLL for (int r = 0; r < 4; ++r) {
                        const float va = V[r][i], vb = V[r][i + j];
                        V[r][i] = sw ? vb : va;
                        V[r][i + j] = sw ? va : vb;
                    }
                }
            }
        }
    }
    RSC_UNROLL for (int r = 0; r < 4; ++r) v[r] = V[r][3];
}

// KeyFrame::UnprojectStereo(i) (KeyFrame.cpp:606-622)
RSC_HD void tri_unproject_stereo(const TriView& K, int i, float (&x3D)[3]) {
    const float z = K.depth[i];
    if (z > 0) {
        const float u = K.kp_raw[2 * i], v = K.kp_raw[2 * i + 1];
        const float xc[3] = {(u - K.cx) * z * K.invfx, (v - K.cy) * z * K.invfy, z};
        RSC_UNROLL for (int r = 0; r < 3; ++r) x3D[r] = tri_dot3(K.Rwc + 3 * r, xc) + K.Ow[r];
    } else {
        x3D[0] = x3D[1] = x3D[2] = 0.0f;
    }
}

// Reprojection gate of one KeyFrame (:339-389).  `mbf_cur` is the CURRENT KeyFrame's mbf for both
// KeyFrames: the reference's right-image error of KeyFrame 2 reads mpCurrentKeyFrame->mbf (:382).
// A NaN error passes (`>` is false), as in the reference.
RSC_HD bool tri_reproj_ok(const TriView& K, const float (&x3D)[3], float z, int idx, float ur, bool stereo,
                          float mbf_cur) {
    const int o = K.octave[idx];
    const float sf = K.scale[o];
    const float sigmaSquare = sf * sf;
    const float x = tri_dot3(K.Rcw, x3D) + K.tcw[0];
    const float y = tri_dot3(K.Rcw + 3, x3D) + K.tcw[1];
    const float invz = (float)(1.0 / (double)z);
    const float kx = K.kp[2 * idx], ky = K.kp[2 * idx + 1];
    const float u = (K.fx * x) * invz + K.cx;
    const float v = (K.fy * y) * invz + K.cy;
    const float errX = u - kx;
    const float errY = v - ky;
    if (!stereo) {
        if ((double)(errX * errX + errY * errY) > 5.991 * (double)sigmaSquare) return false;
    } else {
        const float u_r = u - mbf_cur * invz;
        const float errX_r = u_r - ur;
        if ((double)((errX * errX + errY * errY) + errX_r * errX_r) > 7.8 * (double)sigmaSquare) return false;
    }
    return true;
}

// One matched pair (idx1 in the current KeyFrame K1, idx2 in the neighbour K2): LocalMapping.cpp:262-407.
// Returns the status; x3D is the point where the status is 0 (and whatever the walk had computed otherwise:
// zeros before a point exists).
RSC_HD int32_t tri_pair(const TriView& K1, const TriView& K2, int idx1, int idx2, float (&x3D)[3]) {
    x3D[0] = x3D[1] = x3D[2] = 0.0f;
    const float kp1x = K1.kp[2 * idx1], kp1y = K1.kp[2 * idx1 + 1];
    const float kp2x = K2.kp[2 * idx2], kp2y = K2.kp[2 * idx2 + 1];
    const float kp1_ur = K1.u_right[idx1], kp2_ur = K2.u_right[idx2];
    const bool bStereo1 = kp1_ur >= 0, bStereo2 = kp2_ur >= 0;
    // :274-279 (Rwc = Rcw.transpose(): column r of Rcw)
    const float xn1[3] = {(kp1x - K1.cx) * K1.invfx, (kp1y - K1.cy) * K1.invfy, 1.0f};
    const float xn2[3] = {(kp2x - K2.cx) * K2.invfx, (kp2y - K2.cy) * K2.invfy, 1.0f};
    float ray1[3], ray2[3];
    RSC_UNROLL for (int r = 0; r < 3; ++r) {
        ray1[r] = (K1.Rcw[r] * xn1[0] + K1.Rcw[3 + r] * xn1[1]) + K1.Rcw[6 + r] * xn1[2];
        ray2[r] = (K2.Rcw[r] * xn2[0] + K2.Rcw[3 + r] * xn2[1]) + K2.Rcw[6 + r] * xn2[2];
    }
    const float cosParallaxRays = tri_dot3(ray1, ray2) / (tri_norm3(ray1) * tri_norm3(ray2));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo;
    float cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = K1.cos_stereo[idx1];
    else if (bStereo2) cosParallaxStereo2 = K2.cos_stereo[idx2];  // read ONLY when KeyFrame 1 is not stereo (:287)
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;  // std::min

    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
        (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        // linear triangulation (:296-312)
        float A[4][4];
        RSC_UNROLL for (int c = 0; c < 4; ++c) {
            const float T1r0 = c < 3 ? K1.Rcw[c] : K1.tcw[0], T1r1 = c < 3 ? K1.Rcw[3 + c] : K1.tcw[1];
            const float T1r2 = c < 3 ? K1.Rcw[6 + c] : K1.tcw[2];
            const float T2r0 = c < 3 ? K2.Rcw[c] : K2.tcw[0], T2r1 = c < 3 ? K2.Rcw[3 + c] : K2.tcw[1];
            const float T2r2 = c < 3 ? K2.Rcw[6 + c] : K2.tcw[2];
            A[0][c] = xn1[0] * T1r2 - T1r0;
            A[1][c] = xn1[1] * T1r2 - T1r1;
            A[2][c] = xn2[0] * T2r2 - T2r0;
            A[3][c] = xn2[1] * T2r2 - T2r1;
        }
        float temp[4];
        tri_svd_last_v(A, temp);
        if (temp[3] == 0) return kTriSvdW0;
        x3D[0] = temp[0] / temp[3];
        x3D[1] = temp[1] / temp[3];
        x3D[2] = temp[2] / temp[3];
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        tri_unproject_stereo(K1, idx1, x3D);
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        tri_unproject_stereo(K2, idx2, x3D);
    } else {
        return kTriLowParallax;
    }
    const float z1 = tri_dot3(K1.Rcw + 6, x3D) + K1.tcw[2];
    if (z1 <= 0) return kTriBehind1;
    const float z2 = tri_dot3(K2.Rcw + 6, x3D) + K2.tcw[2];
    if (z2 <= 0) return kTriBehind2;
    if (!tri_reproj_ok(K1, x3D, z1, idx1, kp1_ur, bStereo1, K1.mbf)) return kTriReproj1;
    if (!tri_reproj_ok(K2, x3D, z2, idx2, kp2_ur, bStereo2, K1.mbf)) return kTriReproj2;
    // scale consistency (:392-407)
    const float n1[3] = {x3D[0] - K1.Ow[0], x3D[1] - K1.Ow[1], x3D[2] - K1.Ow[2]};
    const float n2[3] = {x3D[0] - K2.Ow[0], x3D[1] - K2.Ow[1], x3D[2] - K2.Ow[2]};
    const float dist1 = tri_norm3(n1), dist2 = tri_norm3(n2);
    if (dist1 == 0 || dist2 == 0) return kTriZeroDist;
    const float ratioFactor = 1.5f * K1.scale_factor;  // :219
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = K1.scale[K1.octave[idx1]] / K2.scale[K2.octave[idx2]];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return kTriScale;
    return kTriOk;
}

// ---- the driver's host arithmetic -------------------------------------------------------------------

// C = A * B, 3x3 row-major float, every coefficient summed left to right
inline void tri_mul33(const float* A, const float* B, float* C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// LocalMapping::ComputeF12 (LocalMapping.cpp:512-531): T12 = T1w * T2wi (linear parts multiplied, translation
// R1w * t2wi + t1w), t12x = SkewSymmetricMatrix(t12), F12 = K1inv^T * t12x * R12 * K2inv as three 3x3 float
// products left to right.  The product order of an Eigen build is unpinned.
inline void tri_compute_f12(const float* R1w, const float* t1w, const float* R2wi, const float* t2wi, const float* K1inv,
                            const float* K2inv, float* F) {
    float R12[9], t12[3];
    tri_mul33(R1w, R2wi, R12);
    for (int r = 0; r < 3; ++r) t12[r] = tri_dot3(R1w + 3 * r, t2wi) + t1w[r];
    const float t12x[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};
    float K1t[9], M1[9], M2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) K1t[3 * r + c] = K1inv[3 * c + r];
    tri_mul33(K1t, t12x, M1);
    tri_mul33(M1, R12, M2);
    tri_mul33(M2, K2inv, F);
}

// the baseline gate of :232-236: true = the neighbour is skipped
inline bool tri_baseline_short(const float* Ow1, const float* Ow2, float mb2) {
    const float d[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
    return tri_norm3(d) < mb2;
}

#if defined(__HIPCC__)
}  // namespace rsc
#include "rsc_orbmatch.h"
namespace rsc {

// One SearchForTriangulation call (KeyFrame 1 = outer, KeyFrame 2 = inner).
struct TriMatchProblem {
    DevBow A, B;             // the two views' FeatureVectors and descriptors (rsc_bow), by value
    const float2* kp1;       // mvKeysUn of KeyFrame 1 / 2
    const float2* kp2;
    const int32_t* oct2;     // KeyFrame 2 octaves (checked against n_levels on the host)
    const float* scale2;     // KeyFrame 2 mvScaleFactors
    const float* ur1;        // mvuRight
    const float* ur2;
    const float* angle1;     // mvKeysUn angles (orientation check; the rsc_bow views')
    const float* angle2;
    const uint8_t* has1;     // [n1] the slot is skipped: GetMapPoint(idx) != nullptr, or bOnlyStereo and mvuRight < 0
    const uint8_t* has2;     // [n2] the same for KeyFrame 2 (:564-574); the host folds bOnlyStereo in
    float F[9];              // F12 row-major
    float ex, ey;            // tri_epipole
    int4* items;             // [n1 feat entries] (A entry, b0, nb, 0), class 0 | class 1 | class 2   (scratch)
    int32_t* nitems;         // [4] items of each class, common nodes                                  (scratch)
    int32_t* matches12;      // [n1]                                                                    (output)
    uint8_t* den_zero_slot;  // [n1]                                                                    (output)
    int32_t* counts;         // [2] nmatches, den_zero                                                  (output)
};

// One (current KeyFrame, neighbour) pair list of rsc_triangulate_pairs_many.
struct TriPairsProblem {
    TriView K1, K2;
    const int32_t* pairs;  // [npairs][2] (idx1, idx2)
    int32_t npairs;
    int32_t* status;       // [npairs]
    float* x3d;            // [npairs][3]
};

// nodeinfo: kTriMaxFeatures int2 of scratch per problem (the join's node table)
hipError_t launch_search_for_triangulation(int count, const TriMatchProblem* probs, int2* nodeinfo, int check_ori,
                                           hipStream_t st);
hipError_t launch_triangulate_pairs(int count, int max_pairs, const TriPairsProblem* probs, hipStream_t st);
#endif

}  // namespace rsc
