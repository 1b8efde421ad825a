// localproj.hip — Tracking::SearchLocalPoints (src/Tracking.cpp:1003-1028): Frame::isInFrustum
// (src/Frame.cpp:336-392) and ORBmatcher::SearchByProjection(Frame&, vector<MapPoint>&, th)
// (src/ORBmatcher.cpp:16-100) kernels; see rsc_localproj.h for what this matcher sets, the candidate cache
// and the quirks kept, and rsc_projcore.h for the mapping and the fixed-point argument.
#include <hip/hip_runtime.h>
#include "rsc_localproj.h"
#include "rsc_projrounds.h"

namespace rsc {

namespace {

// What the rounds share, one lane per point: grid (points / 256, problems).  fused: isInFrustum runs here
// and its record goes to the caller-visible `track`; else the caller's record is read from there.
__global__ __launch_bounds__(256) void localproj_setup_kernel(const LocalProjProblem* __restrict__ problems,
                                                              int fused, float cos_limit, float th, int keep_max) {
    const LocalProjProblem& Q = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Q.P.n) lp_setup_point(Q, i, fused, cos_limit, th, keep_max);
}

// lp_best by kProjSub lanes.  Each lane keeps its two smallest keys (distance, rank, feature) of
// proj_walk_coop; the two smallest of the subgroup are the best and the runner-up of the streaming update (the
// equivalence proved in tests/test_cpu_localproj.py).  Every lane of the subgroup returns the decision; lanes
// with q.cells < 0 only take part in the shuffles.
__device__ __forceinline__ int lp_best_coop(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP, int i,
                            const int* owner, float nn_ratio, int lane) {
    struct Keys { unsigned long long k1, k2; } k = {kProjNoKey, kProjNoKey};
    if (q.cells >= 0) {
        const ProjStereoGate gate = lp_gate(F, u_right, q);
        const ProjDesc* desc = F.desc;
        k = proj_walk_coop<kProjSub>(F, ProjCells(q.cells), lane, k, [&](Keys s, int f, int rank) {
            if (!gate(f) || owner[f] < i) return s;  // :58-60
            const unsigned long long key = proj_coop_key(proj_desc_dist(dMP, desc[f]), rank, f);
            if (key < s.k1) return Keys{key, s.k1};
            if (key < s.k2) return Keys{s.k1, key};
            return s;
        });
    }
    unsigned long long k1 = k.k1;
    const unsigned long long best = proj_min_coop<kProjSub>(k1);
    if (k1 == best) k1 = k.k2;  // keys are distinct (the rank), so one lane gives up its best
    const unsigned long long second = proj_min_coop<kProjSub>(k1);
    LpTop2 t = lp_top2_init();
    if (best != kProjNoKey) {
        t.bestDist = (int)(best >> 32);
        t.bestIdx = (int)(best & 0xffff);
        t.bestLevel = F.octave[t.bestIdx];
    }
    if (second != kProjNoKey) {
        t.bestDist2 = (int)(second >> 32);
        t.bestLevel2 = F.octave[(int)(second & 0xffff)];
    }
    return lp_decide(t, nn_ratio);
}

struct LpRoundsCoop : LpRounds {
    __device__ int best_coop(int i, bool valid, const int* owner, int lane) const {
        LpRec q;  // read only when valid (lp_best_coop tests cells first)
        q.cells = -1;
        ProjDesc d = {};
        if (valid) {
            q = Q.rec[i];
            d = Q.P.desc[i];
        }
        return lp_best_coop(*Q.F, Q.u_right, q, d, i, owner, nn_ratio, lane);
    }
};

// One workgroup per (Frame, point list) problem.  LDS: the owner table over the Frame's features (32 KB):
// owner[f] = the lowest BLOCKING point (has_obs) that claims f, kProjOccupied for an entry occupant with
// observations; and the list of the points whose cache is exhausted this round (16 KB), whose windows are
// then walked by kProjSub lanes each instead of one (a window at th = 5 holds a hundred features, and one lane
// walking it alone set the length of the whole round).  The points' cached windows, candidates and claims
// live in the problem's scratch (L2-resident), because a local map is larger than the table.
__global__ __launch_bounds__(kLpThreads) void localproj_kernel(const LocalProjProblem* __restrict__ problems,
                                                               float nn_ratio) {
    __shared__ int owner[kLpMaxFeatures];
    __shared__ int walk[kProjWalkCap];
    __shared__ int n_eligible, n_to_match, total;

    const LocalProjProblem& Q = problems[blockIdx.x];
    const DevProjFrame& F = *Q.F;
    const int tid = threadIdx.x;
    const int nF = F.n, nP = Q.P.n;

    if (tid == 0) {
        n_eligible = 0;
        n_to_match = 0;
        total = 0;
    }
    __syncthreads();
    // the points with a window: only they can claim (the bound of the loop below)
    int mine = 0, seen = 0;
    for (int i = tid; i < nP; i += kLpThreads) {
        const LpRec q = Q.rec[i];
        mine += q.cells >= 0;
        seen += q.in_view;
    }
    if (mine) atomicAdd(&n_eligible, mine);
    if (seen) atomicAdd(&n_to_match, seen);
    __syncthreads();

    const int rounds = proj_rounds<kLpThreads>(LpRoundsCoop{{Q, nn_ratio}}, owner, nF, Q.claim, n_eligible, walk);
    // the claims are final: F.mvpMapPoints[f] = the LAST point that took f (:94); every claim counts (:95)
    for (int f = tid; f < nF; f += kLpThreads) owner[f] = -1;
    __syncthreads();
    int cnt = 0;
    for (int i = tid; i < nP; i += kLpThreads) {
        const int a = Q.claim[i];
        if (a < 0) continue;
        atomicMax(&owner[a], i);
        ++cnt;
    }
    if (cnt) atomicAdd(&total, cnt);
    __syncthreads();
    for (int f = tid; f < nF; f += kLpThreads) Q.out[f] = owner[f];
    if (tid == 0) {
        Q.counts[0] = total;
        Q.counts[1] = n_to_match;
        Q.counts[2] = rounds;
    }
}

}  // namespace

hipError_t launch_search_local_points(int count, int max_points, const LocalProjProblem* problems, int fused,
                                      float cos_limit, float th, float nn_ratio, hipEvent_t mid, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    const dim3 g0((max_points + 255) / 256 > 0 ? (max_points + 255) / 256 : 1, count);
    localproj_setup_kernel<<<g0, 256, 0, st>>>(problems, fused, cos_limit, th, lp_keep_max(nn_ratio));
    if (mid) (void)hipEventRecord(mid, st);
    localproj_kernel<<<count, kLpThreads, 0, st>>>(problems, nn_ratio);
    return hipGetLastError();
}

}  // namespace rsc
