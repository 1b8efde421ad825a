// rsc_mpupdate.h — MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cpp:224-289) and
// MapPoint::UpdateNormalAndDepth() (:312-353) over a batch of (point, observation list) records: device layout
// and the arithmetic of one point, shared by mpupdate.hip and the host emulation (tests/mpupdate_emu).
//
// The observation list of a point is the caller's iteration of mObservations, in that order.
//
// ComputeDistinctiveDescriptors, as the reference has it:
//   kept       observations whose KeyFrame isBad() are dropped (:247); N of them remain.  N == 0: nothing is written
//   D[i][j]    the 256-bit Hamming distance of the kept descriptors, D[i][i] = 0 (:257-267)
//   median     of row i: the element of rank (int)(0.5*(N-1)) of the sorted row (:276), the lower median, the
//              diagonal zero being part of the row.  N == 1 and N == 2 both give 0 for every row
//   BestIdx    the first row, in list order, with the strictly smallest median (:278-282)
// No N x N matrix is kept: the element of rank k of a row is the smallest v with |{j : D[i][j] <= v}| > k, found
// by bisection over v in [0, 256] (256, complementary descriptors, is a legal distance): at most 9 passes of
// popcounts over the kept descriptors (mpu_row_median).  The rows of a point are independent; the first strict
// minimum is the smallest key median << 16 | row.
//
// UpdateNormalAndDepth, as the reference has it:
//   all observations count, those of bad KeyFrames included (no isBad() test in :332-339)
//   normali = Pos - Ow_i, normal = normal + normali / normali.norm() in list order from zero: float addition is
//   not associative, so one lane adds; the unit vectors are independent and any lane may form them (mpu_unit)
//   norm() = sqrtf((x*x + y*y) + z*z) (tri_norm3 of rsc_triang.h); the division by it is an IEEE float division
//   per component, not a multiplication by a reciprocal
//   PC = Pos - Ow_ref, dist = PC.norm(), mfMaxDistance = dist * scale[octave_ref], mfMinDistance = mfMaxDistance /
//   scale[n_levels - 1], mNormalVector = normal / (float)n
//   a point on a camera centre gives 0/0: the NaN propagates
// Every operation rounds to float (no contraction: the build passes -ffp-contract=off).
//
// A limit the reference does not have: a list holds at most kMpuMaxObs = 1024 observations (the kept descriptors
// of a point are staged in 32 KB of LDS).  The reference's float Distances[N][N] on the stack overflows an 8 MB
// stack near N = 1400.
#pragma once
#include "rsc_projcore.h"

#ifndef RSC_MPUPDATE_MAX_OBS  // include/rsc.h
#define RSC_MPUPDATE_MAX_OBS 1024
#endif

namespace rsc {

constexpr int kMpuMaxObs = RSC_MPUPDATE_MAX_OBS;
constexpr int kMpuWaveObs = 64;   // lists up to here: one point per wave, lane i owns row i
constexpr int kMpuThreads = 256;  // longer lists: one point per workgroup, rows strided over its lanes
constexpr int kMpuNoKey = 0x7fffffff;

// What the two functions read of a KeyFrame (of an rsc_kfview with rsc_kfview_set_triangulation)
struct MpuKF {
    const ProjDesc* desc;   // [n] mDescriptors rows
    const int32_t* octave;  // [n] mvKeysUn[i].octave
    const float* scale;     // [n_levels] mvScaleFactors
    float Ow[3];            // GetCameraCenter()
    int32_t n_levels;       // mnScaleLevels
};

struct MpuProblem {
    const MpuKF* kfs;
    const float* pos;            // [n_points][3] mWorldPos
    const int32_t* obs_begin;    // [n_points + 1] CSR over the observations
    const int32_t* obs_kf;       // [n_obs] index into kfs
    const int32_t* obs_idx;      // [n_obs] mit->second
    const int32_t* kept_begin;   // [n_points + 1] CSR over the observations of KeyFrames that are not bad
    const int32_t* kept_pos;     // [n_kept] position of the kept observation in its point's list
    const int32_t* ref_kf;       // [n_points] mpRefKF
    const int32_t* ref_idx;      // [n_points] observations[pRefKF]
    const int32_t* dst_index;    // [n_points] slot in the resident view, -1: none; NULL without a view
    const int32_t* order;        // [n_wave + n_block] the points to update: the wave class, then the workgroup class
    ProjDesc* desc;              // [n_points] outputs, written for the updated points only
    int32_t* best_obs;           // [n_points]
    float* normal;               // [n_points][3]
    float* dmax;                 // [n_points]
    float* dmin;                 // [n_points]
    ProjDesc* dst_desc;          // the resident view's arrays (NULL without a view)
    float* dst_normal;
    float* dst_dmax;
    float* dst_dmin;
    int32_t n_wave, n_block;
    int32_t what;                // 1 descriptor | 2 normal and depth
};

// the kept observation k of point p: its position in the point's list, and its descriptor
RSCM_HD int mpu_kept_pos(const MpuProblem& Q, int p, int k) { return Q.kept_pos[Q.kept_begin[p] + k]; }
RSCM_HD const ProjDesc& mpu_obs_desc(const MpuProblem& Q, int p, int pos) {
    const int o = Q.obs_begin[p] + pos;
    return Q.kfs[Q.obs_kf[o]].desc[Q.obs_idx[o]];
}

// :274-276 for the row of `own` without the row: the smallest v in [0, 256] with more than
// (int)(0.5*(N-1)) of the N distances at or below it.  `own` is one of descs, so its zero is counted.
RSCM_HD int mpu_row_median(const ProjDesc& own, const ProjDesc* descs, int N) {
    const int need = (int)(0.5 * (N - 1)) + 1;
    int lo = 0, hi = 256;
    while (lo < hi) {  // 257 values: at most 9 passes
        const int mid = (lo + hi) >> 1;
        int c = 0;
        for (int j = 0; j < N; ++j) c += proj_desc_dist(own, descs[j]) <= mid;
        if (c >= need) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// a strict < in row order is the smallest key
RSCM_HD int mpu_key(int median, int row) { return median << 16 | row; }
RSCM_HD int mpu_key_row(int key) { return key & 0xffff; }

RSCM_HD float mpu_norm3(const float* x) { return sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); }

// normali / normali.norm() (:336-337)
RSCM_HD void mpu_unit(const float* pos, const float* Ow, float* u) {
    const float d[3] = {pos[0] - Ow[0], pos[1] - Ow[1], pos[2] - Ow[2]};
    const float nrm = mpu_norm3(d);
    u[0] = d[0] / nrm;
    u[1] = d[1] / nrm;
    u[2] = d[2] / nrm;
}

// :341-352 given the summed normal: mNormalVector into normal[3], mfMaxDistance, mfMinDistance
RSCM_HD void mpu_finish(const float* pos, const MpuKF& ref, int ref_idx, const float* sum, int n, float* normal,
                        float& dmax, float& dmin) {
    const float pc[3] = {pos[0] - ref.Ow[0], pos[1] - ref.Ow[1], pos[2] - ref.Ow[2]};
    const float dist = mpu_norm3(pc);
    const int level = ref.octave[ref_idx];
    dmax = dist * ref.scale[level];
    dmin = dmax / ref.scale[ref.n_levels - 1];
    const float fn = (float)n;
    normal[0] = sum[0] / fn;
    normal[1] = sum[1] / fn;
    normal[2] = sum[2] / fn;
}

// the outputs of point p, and their copies in the resident view's slot
RSCM_HD void mpu_store_desc(const MpuProblem& Q, int p, int best_obs, const ProjDesc& d) {
    Q.best_obs[p] = best_obs;
    Q.desc[p] = d;
    if (Q.dst_index && Q.dst_index[p] >= 0) Q.dst_desc[Q.dst_index[p]] = d;
}

RSCM_HD void mpu_store_normal(const MpuProblem& Q, int p, const float* normal, float dmax, float dmin) {
    for (int k = 0; k < 3; ++k) Q.normal[3 * p + k] = normal[k];
    Q.dmax[p] = dmax;
    Q.dmin[p] = dmin;
    if (Q.dst_index && Q.dst_index[p] >= 0) {
        const int s = Q.dst_index[p];
        for (int k = 0; k < 3; ++k) Q.dst_normal[3 * s + k] = normal[k];
        Q.dst_dmax[s] = dmax;
        Q.dst_dmin[s] = dmin;
    }
}

#if defined(__HIPCC__)
// one launch per class: grid (n_wave / 4) of one point per wave, grid (n_block) of one point per workgroup
hipError_t launch_mpupdate(const MpuProblem& Q, hipStream_t st);
#endif

}  // namespace rsc
