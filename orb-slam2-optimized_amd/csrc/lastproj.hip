// lastproj.hip — ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th)
// (src/ORBmatcher.cpp:1173-1315) kernels; see rsc_lastproj.h for the mapping, the fixed-point argument, the
// candidate cache, the quirks kept and the nulling rule of the rotation check.
#include <hip/hip_runtime.h>
#include "rsc_lastproj.h"

namespace rsc {

namespace {

// What the rounds share, one lane per LastFrame slot: grid (slots / 256, problems).
__global__ __launch_bounds__(256) void lastproj_setup_kernel(const LastProjProblem* __restrict__ problems, float th) {
    const LastProjProblem& Q = problems[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.L.n) return;
    const DevProjFrame& F = *Q.F;
    LpRec q;
    q.u = q.v = q.r = q.xr = 0.0f;
    q.cells = -1;
    q.in_view = 0;
    q.pad[0] = q.pad[1] = 0;
    ProjCand cd;
    cd.c[0] = cd.c[1] = cd.c[2] = cd.c[3] = -1;
    if (last_eligible(Q.L, i)) {
        q = last_setup(F, Q.mbf, Q.L, Q.Tcw, i, th);
        if (q.cells >= 0) {
            const ProjDesc d = Q.L.mp_desc[i];
            if (last_candidates(F, Q.u_right, q, d, Q.frame_occ, Q.mode, cd)) q.cells |= kProjMore;
        }
    }
    Q.rec[i] = q;
    Q.cand[i] = cd;
    Q.claim[i] = -1;
}

constexpr int kLastSub = 16;                        // lanes that walk one window together
constexpr int kLastSubs = kLastThreads / kLastSub;  // windows walked at a time
constexpr int kLastWalkCap = 4096;                  // LDS list of the slots that walk their window this round

// last_best by kLastSub lanes.  For one column ix the cells iy0..iy1 are contiguous in the CSR (cell = ix * 48
// + iy) and in visiting order, so the lanes stride over each column's entries and every candidate gets its
// rank in the visit.  The smallest (distance, rank) key of the subgroup is the first strict minimum of the
// sequential walk.  Every lane of the subgroup returns the decision; lanes with q.cells < 0 only take part in
// the shuffles.
__device__ int last_best_coop(const DevProjFrame& F, const float* u_right, const LpRec& q, const ProjDesc& dMP, int i,
                              const int* owner, int mode, int lane) {
    const unsigned long long none = ~0ull;
    unsigned long long best = none;
    if (q.cells >= 0) {
        const int x0 = q.cells & 63, x1 = (q.cells >> 6) & 63, y0 = (q.cells >> 12) & 63, y1 = (q.cells >> 18) & 63;
        int lo, hi;
        last_levels(mode, (q.cells >> 24) & 63, lo, hi);
        int rank0 = 0;
        for (int ix = x0; ix <= x1; ++ix) {
            const int b = F.cell_begin[ix * kProjGridRows + y0], e1 = F.cell_begin[ix * kProjGridRows + y1 + 1];
            for (int e = b + lane; e < e1; e += kLastSub) {
                const int f = F.cell_feat[e];
                if (!last_static_gate(F, u_right, q, lo, hi, f)) continue;
                if (owner[f] < i) continue;  // :1248-1250
                const unsigned long long key = (unsigned long long)proj_desc_dist(dMP, F.desc[f]) << 32 |
                                               (unsigned long long)(rank0 + (e - b)) << 16 | (unsigned)f;
                if (key < best) best = key;
            }
            rank0 += e1 - b;
        }
    }
#pragma unroll
    for (int s = kLastSub / 2; s; s >>= 1) {
        const unsigned long long o = __shfl_xor(best, s, kLastSub);
        best = o < best ? o : best;
    }
    if (best == none) return -1;
    return (int)(best >> 32) <= kLpThHigh ? (int)(best & 0xffff) : -1;  // :1271
}

// One workgroup per (current Frame, last Frame) problem.  LDS: the owner table over the current Frame's
// features (32 KB): owner[f] = the lowest BLOCKING slot (has_obs) that claims f, kProjOccupied for an entry
// occupant with observations; the list of the slots whose cache is exhausted this round (16 KB), whose windows
// are then walked by kLastSub lanes each (forward mode has no upper octave, so its windows are the longest);
// and the rotation histogram.  The slots' cached windows, candidates and claims live in the problem's scratch.
__global__ __launch_bounds__(kLastThreads) void lastproj_kernel(const LastProjProblem* __restrict__ problems,
                                                                int check_ori) {
    __shared__ int owner[kLastMaxFeatures];
    __shared__ int walk[kLastWalkCap];
    __shared__ int hist[kProjHistoLength];
    __shared__ int keep[3];
    __shared__ int n_eligible, changed, total, kept, n_walk;

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
    // the slots with a window: only they can claim (the bound of the loop below)
    int mine = 0;
    for (int i = tid; i < nL; i += kLastThreads) mine += Q.rec[i].cells >= 0;
    if (mine) atomicAdd(&n_eligible, mine);
    __syncthreads();

    const int max_rounds = n_eligible + 1;
    int rounds = 0;
    for (int r = 0; r < max_rounds; ++r) {
        for (int f = tid; f < nF; f += kLastThreads) owner[f] = Q.frame_occ[f] == 2 ? kProjOccupied : kProjFree;
        if (tid == 0) {
            changed = 0;
            n_walk = 0;
        }
        __syncthreads();
        for (int i = tid; i < nL; i += kLastThreads) {
            const int a = Q.claim[i];
            if (a >= 0 && Q.L.mp_has_obs[i]) atomicMin(&owner[a], i);  // a slot without observations blocks nobody
        }
        __syncthreads();
        int any = 0;
        for (int i = tid; i < nL; i += kLastThreads) {
            const LpRec q = Q.rec[i];
            if (q.cells < 0) continue;
            const ProjCand cd = Q.cand[i];
            int b = proj_pick(cd, (q.cells & kProjMore) != 0, i, owner);
            if (b == -2) {  // the cached four are taken by lower slots and there were more: walk the window
                const int slot = atomicAdd(&n_walk, 1);
                if (slot < kLastWalkCap) {
                    walk[slot] = i;
                    continue;
                }
                const ProjDesc d = Q.L.mp_desc[i];  // the list is full: alone
                b = last_best(F, Q.u_right, q, d, i, owner, mode);
            }
            if (b != Q.claim[i]) {
                Q.claim[i] = b;
                any = 1;
            }
        }
        __syncthreads();
        const int nw = n_walk < kLastWalkCap ? n_walk : kLastWalkCap;
        const int sub = tid / kLastSub, lane = tid % kLastSub;
        for (int base = 0; base < nw; base += kLastSubs) {  // the same trip count for every lane: shuffles inside
            const int w = base + sub;
            const bool valid = w < nw;
            const int i = valid ? walk[w] : 0;
            LpRec q;
            q.cells = -1;
            ProjDesc d = {};
            if (valid) {
                q = Q.rec[i];
                d = Q.L.mp_desc[i];
            }
            const int b = last_best_coop(F, Q.u_right, q, d, i, owner, mode, lane);
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
