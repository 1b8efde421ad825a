// frameproj.hip — ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) kernel
// (src/ORBmatcher.cpp:1317-1444); see rsc_frameproj.h for the mapping and the fixed-point argument.
#include <hip/hip_runtime.h>
#include "rsc_frameproj.h"

namespace rsc {

namespace {

// What the rounds share, one lane per MapPoint: grid (points / 256, problems).
__global__ __launch_bounds__(256) void frameproj_setup_kernel(const FrameProjProblem* __restrict__ problems, float th,
                                                              int orb_dist) {
    const FrameProjProblem& P = problems[blockIdx.y];
    const DevProjFrame& F = *P.F;
    const DevProjKF& K = P.K;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K.n) return;
    ProjRec q = proj_no_window();
    ProjCand cd;
    cd.c[0] = cd.c[1] = cd.c[2] = cd.c[3] = -1;
    if (proj_eligible(K, P.already, i)) {
        q = proj_setup(F, K, P.Tcw, i, th);
        if (q.cells >= 0) {
            const ProjDesc d = K.mp_desc[i];
            if (proj_candidates(F, q, d, P.frame_mp, orb_dist, cd)) q.cells |= kProjMore;
        }
    }
    P.rec[i] = q;
    P.cand[i] = cd;
    P.claim[i] = -1;
}

// One workgroup per (Frame, KeyFrame) problem.  LDS: the owner table over the Frame's features (32 KB),
// the pre-occupied bits (1 KB) and the rotation histogram; the MapPoints' cached windows, candidates and
// claims live in the problem's scratch (L2-resident, 36 bytes per slot).
__global__ __launch_bounds__(kProjThreads) void frameproj_kernel(const FrameProjProblem* __restrict__ problems,
                                                                 int orb_dist, int check_ori) {
    __shared__ int owner[kProjMaxFeatures];
    __shared__ uint32_t occ[kProjMaxFeatures / 32];
    __shared__ int hist[kProjHistoLength];
    __shared__ int keep[3];
    __shared__ int n_eligible, changed, total;

    const FrameProjProblem& P = problems[blockIdx.x];
    const DevProjFrame& F = *P.F;
    const DevProjKF& K = P.K;
    const int tid = threadIdx.x;
    const int nF = F.n, nK = K.n;

    for (int w = tid; w < kProjMaxFeatures / 32; w += kProjThreads) occ[w] = 0u;
    if (tid < kProjHistoLength) hist[tid] = 0;
    if (tid == 0) {
        n_eligible = 0;
        total = 0;
    }
    __syncthreads();
    for (int f = tid; f < nF; f += kProjThreads) {
        if (P.frame_mp[f] >= 0) atomicOr(&occ[f >> 5], 1u << (f & 31));
        P.out[f] = -1;
    }
    // the MapPoints with a window: only they can claim (the bound of the loop below)
    int mine = 0;
    for (int i = tid; i < nK; i += kProjThreads) mine += P.rec[i].cells >= 0;
    if (mine) atomicAdd(&n_eligible, mine);
    __syncthreads();

    const int max_rounds = n_eligible + 1;
    int rounds = 0;
    for (int r = 0; r < max_rounds; ++r) {
        for (int f = tid; f < nF; f += kProjThreads)
            owner[f] = (occ[f >> 5] >> (f & 31)) & 1u ? kProjOccupied : kProjFree;
        if (tid == 0) changed = 0;
        __syncthreads();
        for (int i = tid; i < nK; i += kProjThreads) {
            const int a = P.claim[i];
            if (a >= 0) atomicMin(&owner[a], i);
        }
        __syncthreads();
        int any = 0;
        for (int i = tid; i < nK; i += kProjThreads) {
            const int cells = P.rec[i].cells;
            if (cells < 0) continue;
            const ProjCand cd = P.cand[i];
            int b = proj_pick(cd, (cells & kProjMore) != 0, i, owner);
            if (b == -2) {  // the cached four are taken and there were more: walk the window
                const ProjDesc d = K.mp_desc[i];
                b = proj_best(F, P.rec[i], d, i, owner, orb_dist);
            }
            if (b != P.claim[i]) {
                P.claim[i] = b;
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

    // rotation histogram (:1405-1415), ComputeThreeMaxima (:1428), removal (:1430-1440)
    if (check_ori) {
        for (int i = tid; i < nK; i += kProjThreads) {
            const int a = P.claim[i];
            if (a < 0 || owner[a] != i) continue;
            const int bin = proj_rot_bin(K.angle[i], F.angle[a]);
            if ((unsigned)bin < (unsigned)kProjHistoLength) atomicAdd(&hist[bin], 1);  // the reference asserts it
        }
        __syncthreads();
        if (tid == 0) {
            int hs[kProjHistoLength];
#pragma unroll
            for (int b = 0; b < kProjHistoLength; ++b) hs[b] = hist[b];
            const int m = proj_three_maxima(hs, kProjHistoLength);
            keep[0] = (m & 255) - 1;
            keep[1] = ((m >> 8) & 255) - 1;
            keep[2] = ((m >> 16) & 255) - 1;
        }
        __syncthreads();
    }
    int cnt = 0;
    for (int i = tid; i < nK; i += kProjThreads) {
        const int a = P.claim[i];
        if (a < 0 || owner[a] != i) continue;
        if (check_ori) {
            const int bin = proj_rot_bin(K.angle[i], F.angle[a]);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) continue;
        }
        P.out[a] = i;
        ++cnt;
    }
    if (cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) {
        *P.nmatches = total;
        *P.rounds = rounds;
    }
}

}  // namespace

hipError_t launch_search_by_projection(int count, int max_kf_points, const FrameProjProblem* problems, float th,
                                       int orb_dist, int check_orientation, hipStream_t st) {
    const dim3 g0((max_kf_points + 255) / 256 > 0 ? (max_kf_points + 255) / 256 : 1, count);
    frameproj_setup_kernel<<<g0, 256, 0, st>>>(problems, th, orb_dist);
    frameproj_kernel<<<count, kProjThreads, 0, st>>>(problems, orb_dist, check_orientation);
    return hipGetLastError();
}

}  // namespace rsc
