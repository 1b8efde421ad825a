// frameproj.hip — ORBmatcher::SearchByProjection(Frame&, KeyFrame, sAlreadyFound, th, ORBdist) kernel
// (src/ORBmatcher.cpp:1317-1444); see rsc_frameproj.h for what this matcher sets and rsc_projcore.h for the
// mapping and the fixed-point argument.
#include <hip/hip_runtime.h>
#include "rsc_frameproj.h"
#include "rsc_projrounds.h"

namespace rsc {

namespace {

// What the rounds share, one lane per MapPoint: grid (points / 256, problems).
__global__ __launch_bounds__(256) void frameproj_setup_kernel(const FrameProjProblem* __restrict__ problems, float th,
                                                              int orb_dist) {
    const FrameProjProblem& P = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P.K.n) proj_setup_point(P, i, th, orb_dist);
}

// the pre-occupied bits in LDS
struct ProjOccBits {
    const uint32_t* w;
    RSCM_HD bool operator()(int f) const { return (w[f >> 5] >> (f & 31)) & 1u; }
};

// One workgroup per (Frame, KeyFrame) problem.  LDS: the owner table over the Frame's features (32 KB),
// the pre-occupied bits (1 KB) and the rotation histogram; the MapPoints' cached windows, candidates and
// claims live in the problem's scratch (L2-resident, 36 bytes per slot).
__global__ __launch_bounds__(kProjThreads) void frameproj_kernel(const FrameProjProblem* __restrict__ problems,
                                                                 int orb_dist, int check_ori) {
    __shared__ int owner[kProjMaxFeatures];
    __shared__ uint32_t occ[kProjMaxFeatures / 32];
    __shared__ int hist[kProjHistoLength];
    __shared__ int keep[3];
    __shared__ int n_eligible, total;

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
    proj_count_eligible<kProjThreads>(P.rec, nK, &n_eligible);
    __syncthreads();

    const int rounds = proj_rounds<kProjThreads>(FrameRounds<ProjOccBits>{P, orb_dist, ProjOccBits{occ}}, owner, nF,
                                                 P.claim, n_eligible, nullptr);
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
            int hs[kProjHistoLength], k3[3];
#pragma unroll
            for (int b = 0; b < kProjHistoLength; ++b) hs[b] = hist[b];
            proj_keep_bins(hs, k3);
            keep[0] = k3[0];
            keep[1] = k3[1];
            keep[2] = k3[2];
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
