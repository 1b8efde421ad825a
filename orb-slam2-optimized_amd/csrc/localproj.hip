// localproj.hip — Tracking::SearchLocalPoints (src/Tracking.cpp:1003-1028): Frame::isInFrustum
// (src/Frame.cpp:336-392) and ORBmatcher::SearchByProjection(Frame&, vector<MapPoint>&, th)
// (src/ORBmatcher.cpp:16-100) kernels; see rsc_localproj.h for the mapping, the fixed-point argument, the
// candidate cache and the quirks kept.
#include <hip/hip_runtime.h>
#include "rsc_localproj.h"

namespace rsc {

namespace {

// What the rounds share, one lane per point: grid (points / 256, problems).  fused: isInFrustum runs here
// and its record goes to the caller-visible `track`; else the caller's record is read from there.
__global__ __launch_bounds__(256) void localproj_setup_kernel(const LocalProjProblem* __restrict__ problems,
                                                              int fused, float cos_limit, float th, int keep_max) {
    const LocalProjProblem& Q = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.P.n) return;
    const DevProjFrame& F = *Q.F;
    LpTrack t = lp_not_in_view();
    const bool eligible = lp_eligible(Q.P, Q.skip, i);
    if (fused) {
        if (eligible) t = lp_frustum(F, Q.mbf, Q.P, Q.Tcw, i, cos_limit);
        Q.track[i] = t;
    } else if (eligible) {
        t = Q.track[i];
        if ((unsigned)t.level >= (unsigned)F.n_levels) t.in_view = 0;  // the host checked it; never index past scale[]
    }
    LpRec q = lp_window(F, t, th);
    ProjCand cd;
    cd.c[0] = cd.c[1] = cd.c[2] = cd.c[3] = -1;
    if (q.cells >= 0) {
        const ProjDesc d = Q.P.desc[i];
        if (lp_candidates(F, Q.u_right, q, d, Q.frame_occ, keep_max, cd)) q.cells |= kProjMore;
    }
    Q.rec[i] = q;
    Q.cand[i] = cd;
    Q.claim[i] = -1;
}

constexpr int kLpSub = 16;                      // lanes that walk one window together
constexpr int kLpSubs = kLpThreads / kLpSub;    // windows walked at a time
constexpr int kLpWalkCap = 4096;                // LDS list of the points that walk their window this round

// lp_best by kLpSub lanes.  For one column ix the cells iy0..iy1 are contiguous in the CSR (cell = ix * 48 +
// iy) and in visiting order, so the lanes stride over each column's entries and every candidate gets its rank
// in the visit.  Each lane keeps its two smallest keys (distance, rank, feature); the two smallest of the
// subgroup are the best and the runner-up of the streaming update (the equivalence proved in
// tests/test_cpu_localproj.py).  Every lane of the subgroup returns the decision; lanes with q.cells < 0 only
// take part in the shuffles.
__device__ int lp_best_coop(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP, int i,
                            const int* owner, float nn_ratio, int lane) {
    const unsigned long long none = ~0ull;
    unsigned long long k1 = none, k2 = none;
    if (q.cells >= 0) {
        const int x0 = q.cells & 63, x1 = (q.cells >> 6) & 63, y0 = (q.cells >> 12) & 63, y1 = (q.cells >> 18) & 63;
        const int level = (q.cells >> 24) & 63;
        int rank0 = 0;
        for (int ix = x0; ix <= x1; ++ix) {
            const int b = F.cell_begin[ix * kProjGridRows + y0], e1 = F.cell_begin[ix * kProjGridRows + y1 + 1];
            for (int e = b + lane; e < e1; e += kLpSub) {
                const int f = F.cell_feat[e];
                if (!lp_static_gate(F, u_right, q, level, f)) continue;
                if (owner[f] < i) continue;  // :58-60
                const unsigned long long key = (unsigned long long)proj_desc_dist(dMP, F.desc[f]) << 32 |
                                               (unsigned long long)(rank0 + (e - b)) << 16 | (unsigned)f;
                if (key < k1) {
                    k2 = k1;
                    k1 = key;
                } else if (key < k2) {
                    k2 = key;
                }
            }
            rank0 += e1 - b;
        }
    }
    unsigned long long best = k1;
#pragma unroll
    for (int s = kLpSub / 2; s; s >>= 1) {
        const unsigned long long o = __shfl_xor(best, s, kLpSub);
        best = o < best ? o : best;
    }
    if (k1 == best) {  // keys are distinct (the rank), so one lane gives up its best
        k1 = k2;
        k2 = none;
    }
    unsigned long long second = k1;
#pragma unroll
    for (int s = kLpSub / 2; s; s >>= 1) {
        const unsigned long long o = __shfl_xor(second, s, kLpSub);
        second = o < second ? o : second;
    }
    LpTop2 t = lp_top2_init();
    if (best != none) {
        t.bestDist = (int)(best >> 32);
        t.bestIdx = (int)(best & 0xffff);
        t.bestLevel = F.octave[t.bestIdx];
    }
    if (second != none) {
        t.bestDist2 = (int)(second >> 32);
        t.bestLevel2 = F.octave[(int)(second & 0xffff)];
    }
    return lp_decide(t, nn_ratio);
}

// One workgroup per (Frame, point list) problem.  LDS: the owner table over the Frame's features (32 KB):
// owner[f] = the lowest BLOCKING point (has_obs) that claims f, kProjOccupied for an entry occupant with
// observations; and the list of the points whose cache is exhausted this round (16 KB), whose windows are
// then walked by kLpSub lanes each instead of one (a window at th = 5 holds a hundred features, and one lane
// walking it alone set the length of the whole round).  The points' cached windows, candidates and claims
// live in the problem's scratch (L2-resident), because a local map is larger than the table.
__global__ __launch_bounds__(kLpThreads) void localproj_kernel(const LocalProjProblem* __restrict__ problems,
                                                               float nn_ratio) {
    __shared__ int owner[kLpMaxFeatures];
    __shared__ int walk[kLpWalkCap];
    __shared__ int n_eligible, n_to_match, changed, total, n_walk;

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

    const int max_rounds = n_eligible + 1;
    int rounds = 0;
    for (int r = 0; r < max_rounds; ++r) {
        for (int f = tid; f < nF; f += kLpThreads) owner[f] = Q.frame_occ[f] == 2 ? kProjOccupied : kProjFree;
        if (tid == 0) {
            changed = 0;
            n_walk = 0;
        }
        __syncthreads();
        for (int i = tid; i < nP; i += kLpThreads) {
            const int a = Q.claim[i];
            if (a >= 0 && Q.has_obs[i]) atomicMin(&owner[a], i);  // a point without observations blocks nobody
        }
        __syncthreads();
        int any = 0;
        for (int i = tid; i < nP; i += kLpThreads) {
            const LpRec q = Q.rec[i];
            if (q.cells < 0) continue;
            const ProjCand cd = Q.cand[i];
            int b = lp_pick(F, cd, (q.cells & kProjMore) != 0, i, owner, nn_ratio);
            if (b == -2) {  // fewer than two cached candidates are free and there were more: walk the window
                const int slot = atomicAdd(&n_walk, 1);
                if (slot < kLpWalkCap) {
                    walk[slot] = i;
                    continue;
                }
                const ProjDesc d = Q.P.desc[i];  // the list is full: alone
                b = lp_best(F, Q.u_right, q, d, i, owner, nn_ratio);
            }
            if (b != Q.claim[i]) {
                Q.claim[i] = b;
                any = 1;
            }
        }
        __syncthreads();
        const int nw = n_walk < kLpWalkCap ? n_walk : kLpWalkCap;
        const int sub = tid / kLpSub, lane = tid % kLpSub;
        for (int base = 0; base < nw; base += kLpSubs) {  // the same trip count for every lane: shuffles inside
            const int w = base + sub;
            const bool valid = w < nw;
            const int i = valid ? walk[w] : 0;
            LpRec q;
            q.cells = -1;
            ProjDesc d = {};
            if (valid) {
                q = Q.rec[i];
                d = Q.P.desc[i];
            }
            const int b = lp_best_coop(F, Q.u_right, q, d, i, owner, nn_ratio, lane);
            if (valid && lane == 0 && b != Q.claim[i]) {
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
