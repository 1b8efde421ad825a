// kfproj.hip — ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:241-352)
// and ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:823-946) kernels; see rsc_kfproj.h for the
// mapping, the fixed-point argument and the quirks kept.
#include <hip/hip_runtime.h>
#include "rsc_kfproj.h"

namespace rsc {

namespace {

// What the rounds share, one lane per point: grid (points / 256, problems).
__global__ __launch_bounds__(256) void kfproj_setup_kernel(const KfProjProblem* __restrict__ problems, float th) {
    const KfProjProblem& Q = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.P.n) return;
    ProjRec q = proj_no_window();
    ProjCand cd;
    cd.c[0] = cd.c[1] = cd.c[2] = cd.c[3] = -1;
    if (kfp_eligible(Q.P, Q.already, i)) {
        float R[9], t[3];
        kfp_decompose(Q.Scw, false, R, t);
        q = kfp_setup(Q.K, Q.P, R, t, i, th, false);
        if (q.cells >= 0) {
            const ProjDesc d = Q.P.desc[i];
            if (kfp_candidates(Q.K, q, d, Q.occupied, cd)) q.cells |= kProjMore;
        }
    }
    Q.rec[i] = q;
    Q.cand[i] = cd;
    Q.claim[i] = -1;
}

// One workgroup per (KeyFrame, point set) problem.  LDS: the owner table over the KeyFrame's keypoints
// (32 KB); the points' cached windows, candidates and claims live in the problem's scratch (L2-resident,
// 36 bytes per point), because a point set can be larger than the table.
__global__ __launch_bounds__(kKfpThreads) void kfproj_kernel(const KfProjProblem* __restrict__ problems) {
    __shared__ int owner[kKfpMaxKeypoints];
    __shared__ int n_eligible, changed, total;

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
    // the points with a window: only they can claim (the bound of the loop below)
    int mine = 0;
    for (int i = tid; i < nP; i += kKfpThreads) mine += Q.rec[i].cells >= 0;
    if (mine) atomicAdd(&n_eligible, mine);
    __syncthreads();

    const int max_rounds = n_eligible + 1;
    int rounds = 0;
    for (int r = 0; r < max_rounds; ++r) {
        for (int f = tid; f < nK; f += kKfpThreads) owner[f] = Q.occupied[f] ? kProjOccupied : kProjFree;
        if (tid == 0) changed = 0;
        __syncthreads();
        for (int i = tid; i < nP; i += kKfpThreads) {
            const int a = Q.claim[i];
            if (a >= 0) atomicMin(&owner[a], i);
        }
        __syncthreads();
        int any = 0;
        for (int i = tid; i < nP; i += kKfpThreads) {
            const ProjRec q = Q.rec[i];
            if (q.cells < 0) continue;
            const ProjCand cd = Q.cand[i];
            int b = proj_pick(cd, (q.cells & kProjMore) != 0, i, owner);
            if (b == -2) {  // the cached four are taken and there were more: walk the window
                const ProjDesc d = Q.P.desc[i];
                b = kfp_best(K, q, d, i, owner);
            }
            if (b != Q.claim[i]) {
                Q.claim[i] = b;
                any = 1;
            }
        }
        if (any) changed = 1;
        ++rounds;
        __syncthreads();
        const int go = changed;
        __syncthreads();
        if (!go) break;
    }
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
