// kfproj.hip — ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:241-352)
// and ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:823-946) kernels; see rsc_kfproj.h for the
// quirks kept and what this matcher sets, and rsc_projcore.h for the mapping and the fixed-point argument.
#include <hip/hip_runtime.h>
#include "rsc_kfproj.h"
#include "rsc_projrounds.h"

namespace rsc {

namespace {

// What the rounds share, one lane per point: grid (points / 256, problems).
__global__ __launch_bounds__(256) void kfproj_setup_kernel(const KfProjProblem* __restrict__ problems, float th) {
    const KfProjProblem& Q = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Q.P.n) kfp_setup_point(Q, i, th);
}

// One workgroup per (KeyFrame, point set) problem.  LDS: the owner table over the KeyFrame's keypoints
// (32 KB); the points' cached windows, candidates and claims live in the problem's scratch (L2-resident,
// 36 bytes per point), because a point set can be larger than the table.
__global__ __launch_bounds__(kKfpThreads) void kfproj_kernel(const KfProjProblem* __restrict__ problems) {
    __shared__ int owner[kKfpMaxKeypoints];
    __shared__ int n_eligible, total;

    const KfProjProblem& Q = problems[blockIdx.x];
    const DevKfpKF& K = Q.K;
    const int tid = threadIdx.x;
    const int nK = K.n, nP = Q.P.n;

    if (tid == 0) {
        n_eligible = 0;
        total = 0;
    }
    __syncthreads();
    for (int f = tid; f < nK; f += kKfpThreads) Q.out[f] = -1;
    proj_count_eligible<kKfpThreads>(Q.rec, nP, &n_eligible);
    __syncthreads();

    const int rounds = proj_rounds<kKfpThreads>(KfpRounds{Q}, owner, nK, Q.claim, n_eligible, nullptr);
    // `owner` is the table of the final claims (the last round changed none): owner[A[i]] == i
    int cnt = 0;
    for (int i = tid; i < nP; i += kKfpThreads) {
        const int a = Q.claim[i];
        if (a < 0 || owner[a] != i) continue;
        Q.out[a] = i;  // vpMatched[bestIdx] = pMP (:345)
        ++cnt;
    }
    if (cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) {
        *Q.nmatches = total;
        *Q.rounds = rounds;
    }
}

// Fuse: one lane per (point, KeyFrame) pair, grid (points / 256, KeyFrames).
__global__ __launch_bounds__(256) void kffuse_kernel(const KfFuseProblem* __restrict__ problems, DevKfpPoints P,
                                                     float th) {
    const KfFuseProblem& Q = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    Q.best_idx[i] = kfp_fuse_point(Q.K, P, Q.Scw, Q.in_kf, i, th);
}

}  // namespace

hipError_t launch_search_by_projection_kf(int count, int max_points, const KfProjProblem* problems, float th,
                                          hipStream_t st) {
    const dim3 g0((max_points + 255) / 256 > 0 ? (max_points + 255) / 256 : 1, count);
    kfproj_setup_kernel<<<g0, 256, 0, st>>>(problems, th);
    kfproj_kernel<<<count, kKfpThreads, 0, st>>>(problems);
    return hipGetLastError();
}

hipError_t launch_fuse_sim3(int count, const DevKfpPoints* points, int n_points, const KfFuseProblem* problems,
                            float th, hipStream_t st) {
    if (n_points <= 0 || count <= 0) return hipSuccess;
    const dim3 g((n_points + 255) / 256, count);
    kffuse_kernel<<<g, 256, 0, st>>>(problems, *points, th);
    return hipGetLastError();
}

}  // namespace rsc
