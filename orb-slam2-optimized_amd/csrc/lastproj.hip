// lastproj.hip — ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
// (src/ORBmatcher.cpp:1173-1315) kernels; see rsc_lastproj.h for what this matcher sets, the candidate cache,
// the quirks kept and the nulling rule of the rotation check, and rsc_projcore.h for the mapping and the
// fixed-point argument.
#include <hip/hip_runtime.h>
#include "rsc_lastproj.h"
#include "rsc_projrounds.h"

namespace rsc {

namespace {

// What the rounds share, one lane per LastFrame slot: grid (slots / 256, problems).
__global__ __launch_bounds__(256) void lastproj_setup_kernel(const LastProjProblem* __restrict__ problems, float th) {
    const LastProjProblem& Q = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Q.L.n) last_setup_slot(Q, i, th);
}

struct LastRoundsCoop : LastRounds {
    __device__ int best_coop(int i, bool valid, const int* owner, int lane) const {
        LpRec q = lp_no_window();
        ProjDesc d = {};
        if (valid) {
            q = Q.rec[i];
            d = Q.L.mp_desc[i];
        }
        return proj_first_min_coop<kProjSub>(*Q.F, q.cells, d, i, owner, last_gate(*Q.F, Q.u_right, q, mode),
                                             kLpThHigh, lane);
    }
};

// One workgroup per (current Frame, last Frame) problem.  LDS: the owner table over the current Frame's
// features (32 KB): owner[f] = the lowest BLOCKING slot (has_obs) that claims f, kProjOccupied for an entry
// occupant with observations; the list of the slots whose cache is exhausted this round (16 KB), whose windows
// are then walked by kProjSub lanes each (forward mode has no upper octave, so its windows are the longest);
// and the rotation histogram.  The slots' cached windows, candidates and claims live in the problem's scratch.
__global__ __launch_bounds__(kLastThreads) void lastproj_kernel(const LastProjProblem* __restrict__ problems,
                                                                int check_ori) {
    __shared__ int owner[kLastMaxFeatures];
    __shared__ int walk[kProjWalkCap];
    __shared__ int hist[kProjHistoLength];
    __shared__ int keep[3];
    __shared__ int n_eligible, total, kept;

    const LastProjProblem& Q = problems[blockIdx.x];
    const DevProjFrame& F = *Q.F;
    const int tid = threadIdx.x;
    const int nF = F.n, nL = Q.L.n;
    const int mode = Q.mode;

    if (tid < kProjHistoLength) hist[tid] = 0;
    if (tid == 0) {
        n_eligible = 0;
        total = 0;
        kept = 0;
    }
    __syncthreads();
    proj_count_eligible<kLastThreads>(Q.rec, nL, &n_eligible);
    __syncthreads();

    const int rounds = proj_rounds<kLastThreads>(LastRoundsCoop{{Q, mode}}, owner, nF, Q.claim, n_eligible, walk);
    // The claims are final.  Rotation histogram over ALL claims (:1276-1286), ComputeThreeMaxima (:1299)
    if (check_ori) {
        for (int i = tid; i < nL; i += kLastThreads) {
            const int a = Q.claim[i];
            if (a < 0) continue;
            const int bin = proj_rot_bin(Q.L.angle[i], F.angle[a]);
            if ((unsigned)bin < (unsigned)kProjHistoLength) atomicAdd(&hist[bin], 1);  // the reference asserts it
        }
        __syncthreads();
        if (tid == 0) {
            int hs[kProjHistoLength], k3[3];
#pragma unroll
            for (int b = 0; b < kProjHistoLength; ++b) hs[b] = hist[b];
            last_keep_bins(hs, k3);
            keep[0] = k3[0];
            keep[1] = k3[1];
            keep[2] = k3[2];
        }
    }
    // mvpMapPoints[f] = the LAST slot that took f (:1273); every claim counts (:1274)
    for (int f = tid; f < nF; f += kLastThreads) owner[f] = -1;
    __syncthreads();
    int cnt = 0;
    for (int i = tid; i < nL; i += kLastThreads) {
        const int a = Q.claim[i];
        if (a < 0) continue;
        atomicMax(&owner[a], i);
        ++cnt;
    }
    if (cnt) atomicAdd(&total, cnt);
    __syncthreads();
    // the removal (:1301-1311) runs per histogram entry: ANY claimer of f in a removed bin nulls f
    int good = 0;
    for (int i = tid; i < nL; i += kLastThreads) {
        const int a = Q.claim[i];
        if (a < 0) continue;
        if (check_ori) {
            const int bin = proj_rot_bin(Q.L.angle[i], F.angle[a]);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) {
                owner[a] = kLastNulled;  // every writer of this phase stores the same value
                continue;
            }
        }
        ++good;
    }
    if (good) atomicAdd(&kept, good);
    __syncthreads();
    for (int f = tid; f < nF; f += kLastThreads) Q.out[f] = owner[f];
    if (tid == 0) {
        Q.counts[0] = kept;
        Q.counts[1] = mode;
        Q.counts[2] = rounds;
        Q.counts[3] = total;
    }
}

}  // namespace

hipError_t launch_search_by_projection_last(int count, int max_slots, const LastProjProblem* problems, float th,
                                            int check_orientation, hipEvent_t mid, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    const dim3 g0((max_slots + 255) / 256 > 0 ? (max_slots + 255) / 256 : 1, count);
    lastproj_setup_kernel<<<g0, 256, 0, st>>>(problems, th);
    if (mid) (void)hipEventRecord(mid, st);
    lastproj_kernel<<<count, kLastThreads, 0, st>>>(problems, check_orientation);
    return hipGetLastError();
}

}  // namespace rsc
